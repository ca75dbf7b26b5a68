"""ctypes binding of the HIP library (``csrc/libgobblet_hip.so``, C-ABI in ``include/gobblet_hip.h``).

There is no CPU fallback: if the library cannot be built or loaded this module raises.
``import torch`` happens first on purpose -- the PyTorch-ROCm wheel bundles the HIP runtime
under the same SONAME (``libamdhip64.so.7``) the library links against, so importing torch
first makes the process use ONE runtime and lets torch streams / tensors be handed across
the ABI as plain pointers.
"""
from __future__ import annotations

import ctypes as C
import fcntl
import os
import platform
import shutil
import subprocess

import torch  # noqa: F401  (must precede loading the HIP library, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libgobblet_hip.so")
_FOREIGN = False  # use_library() was called: LIB_PATH is somebody's own build, never rebuilt from here
SOURCES = [os.path.join(CSRC, "gobblet_hip.hip"), os.path.join(CSRC, "gobblet_device.h"), os.path.join(CSRC, "gobblet_diag.h"),
           os.path.join(CSRC, "gobblet_knobs.h"), os.path.join(CSRC, "gobblet_selfplay_entries.inc"),
           os.path.join(CSRC, "gobblet_env_entries.inc"), os.path.join(_HERE, "..", "include", "gobblet_hip.h")]
# -amdgpu-kernarg-preload-count: the first 16 dwords of a kernel's arguments arrive in SGPRs with the wave
# launch (the kernels order their arguments for that), so a wavefront's first loads do not wait for a
# kernel-argument fetch; firmware without the feature runs the compiler's fallback prologue
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-mcode-object-version=5",
               "-mllvm", "-amdgpu-kernarg-preload-count=16"]

OK, ERR_ARG, ERR_ALIGN, ERR_HIP = 0, -1, -2, -3
ILLEGAL_NOOP, ILLEGAL_TERMINATE = 0, 1
POLICY_RANDOM, POLICY_GREEDY1, POLICY_GREEDY2, POLICY_GREEDY3 = 0, 1, 2, 3  # gbl_collect_policy
HOW_RANDOM, HOW_GREEDY, HOW_FALLBACK = 0, 1, 2
POLICY_TREE, HOW_SEARCH, HOW_SEARCH_SAMPLED, Z_OPEN = 4, 3, 4, -128  # gbl_collect_search / gbl_outcome_targets
POLICY_EVAL_TREE = 5  # gbl_collect_search_eval
SOLVE_MAX_DEPTH, SOLVE_NONE = 6, -128  # gbl_solve
HOW_PROVEN = 5  # gbl_collect_search_solve
STREAM_NOISE, NOISE_MAX_WEIGHT = 6, 256  # gbl_tree_search_eval_noise / gbl_collect_search_noise
POLICY_TABLEBASE, HOW_TABLE, HOW_TABLE_SAMPLED = 6, 6, 7  # gbl_collect_search_tb
HOW_FAST, HOW_FAST_SAMPLED, STREAM_CAP, CAP_FULL_SHARE = 8, 9, 9, 256  # gbl_collect_search_cap
HOW_GUMBEL, STREAM_GUMBEL = 10, 10  # gbl_tree_search_gumbel / gbl_collect_search_gumbel
SYMMETRIES, BATCH_ATTEMPTS = 512, 16  # gbl_symmetry_apply / gbl_training_batch
REPLAY_OBS_PITCH, REPLAY_VISITS_PITCH, REPLAY_META_PITCH = 128, 64, 64  # gbl_replay_append / gbl_replay_batch: the ring's row pitches
REPLAY_META_Z, REPLAY_META_MOVER, REPLAY_META_TAG, STREAM_REPLAY = 54, 55, 56, 7
STREAM_REPLAY_PRIO = 8  # gbl_replay_batch_prio's draws
TB_TERMINAL, TB_MAX_SWEEP, TB_AUX_BYTES = -128, 126, 63120  # gbl_tb_*
TB_TARGET_MODES, TB_TARGET_MAX_COUNT = {"result": 0, "shortest": 1}, 600  # gbl_tb_targets
STATUS_ILLEGAL, STATUS_OUT_OF_RANGE = 1, 2  # gbl_step_ex / gbl_collect_from_ex status bits
CELLS, ACTIONS, OBS_BYTES = 27, 54, 117
COUNTER_STRIPES, COUNTER_STRIDE = 64, 16
# gbl_board_eval record (include/gobblet_hip.h GBL_REC_*): field -> (byte offset, bytes)
REC_BYTES = 432
REC_FIELDS = {"squares": (0, 27), "winner": (28, 1), "flat": (32, 9), "covered": (44, 27), "mask0": (72, 54),
              "mask1": (128, 54), "obs0": (184, 117), "obs1": (304, 117)}

_vp, _i64, _u64, _u32, _int = C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_int


def _args(ctype, *names):
    return tuple((name, ctype) for name in names)


# The self-play family's argument lists, BY NAME, from the blocks include/gobblet_hip.h builds its seven declarations of:
# symbol -> ((parameter name, ctype), ...) in the ABI's order.  SIGNATURES below, selfplay_call(), collect(), the tests' harness and
# scripts/record_selfplay_arg_errors.py all take the order from here; tests/test_abi_and_host.py holds it against the header.
_BOARDS = _args(_vp, "state", "to_move", "done")
_TRAJ = _args(_vp, "actions_traj", "winner_traj", "reward_traj", "done_traj", "to_move_traj", "mask_traj", "obs_traj", "visits_traj",
              "value_traj", "nodes_traj", "how_traj", "mover_traj")
_TRAJ_EVAL = _TRAJ + _args(_vp, "root_value_traj", "priors_traj")   # (the evaluator search's two)
_TRAJ_SOLVE = _TRAJ_EVAL + _args(_vp, "outcome_traj", "proven_traj")  # (the guard's two)
_WINDOW = (("n", _i64), ("ply_stride", _i64), ("tile_stride", _i64), ("seed", _u64), ("env_base", _u64), ("ply0", _u32), ("ply_dev", _vp),
           ("plies", _u32), ("policy0", _int), ("policy1", _int))
_SIDES_EVAL = _args(_vp, "ev0", "ev1") + _args(_int, "iterations0", "iterations1")
_SIDES_SOLVE = _SIDES_EVAL + _args(_int, "solve_depth0", "solve_depth1")
_SIDES_NOISE = _SIDES_SOLVE + _args(_int, "noise0", "noise1")
_TAIL = _args(_int, "explore", "sample_plies", "illegal_mode") + _args(_vp, "counters", "turn")
_STREAM = _args(_vp, "stream")
_TABLE = _args(_vp, "inventory", "aux", "table") + _args(_int, "tb_mode", "tb_count") + \
    _args(_vp, "tb_outcome_traj", "tb_value_traj", "tb_played_traj")  # (the table as gbl_tb_probe takes it, its mode and count, the judge's three)
SELFPLAY_ARGS = {
    "gbl_collect_search": _BOARDS + _TRAJ + _WINDOW + _args(_int, "iterations0", "iterations1", "playouts0", "playouts1", "max_plies") +
                          _TAIL + _STREAM,
    "gbl_collect_search_eval": _BOARDS + _TRAJ_EVAL + _WINDOW + _SIDES_EVAL + _TAIL + _STREAM,
    "gbl_collect_search_solve": _BOARDS + _TRAJ_SOLVE + _WINDOW + _SIDES_SOLVE + _TAIL + _STREAM,
    "gbl_collect_search_noise": _BOARDS + _TRAJ_SOLVE + _WINDOW + _SIDES_NOISE + _TAIL + _STREAM,
    "gbl_collect_search_cap": _BOARDS + _TRAJ_SOLVE + _WINDOW + _SIDES_NOISE + _TAIL +
                              _args(_int, "fast_iterations0", "fast_iterations1", "full_share0", "full_share1") + _STREAM,
    "gbl_collect_search_gumbel": _BOARDS + _TRAJ_EVAL + _WINDOW + _SIDES_EVAL + _TAIL +
                                 _args(_int, "considered0", "considered1", "gumbel_noise", "visit_offset", "scale") + _STREAM,
    "gbl_collect_search_tb": _BOARDS + _TRAJ_SOLVE + _WINDOW + _SIDES_NOISE + _TAIL + _TABLE + _STREAM,
}
_GUMBEL = _args(_int, "considered0", "considered1", "gumbel_noise", "visit_offset", "scale")
# ... and the self-play entry points outside the gbl_collect_search* names, from the same blocks: selfplay_args() / selfplay_call() look
# in every table; tests/test_gumbel_solve.py holds this one against both headers.
SELFPLAY_ARGS_MORE = {
    "gbl_collect_gumbel_solve": _BOARDS + _TRAJ_SOLVE + _WINDOW + _SIDES_SOLVE + _TAIL + _GUMBEL + _STREAM,
}
# ... and beside it the Gumbel window with the table: gbl_collect_search_gumbel's arguments up to `scale`, then gbl_collect_search_tb's
# table block; tests/test_gumbel_tb.py holds it against both headers.
SELFPLAY_ARGS_TABLE = {
    "gbl_collect_gumbel_tb": _BOARDS + _TRAJ_EVAL + _WINDOW + _SIDES_EVAL + _TAIL + _GUMBEL + _TABLE + _STREAM,
}
_SELFPLAY_TABLES = (SELFPLAY_ARGS, SELFPLAY_ARGS_MORE, SELFPLAY_ARGS_TABLE)


def selfplay_table(entry: str) -> tuple:
    """``entry``'s ((parameter name, ctype), ...) in the ABI's order, from whichever of the tables has it."""
    for table in _SELFPLAY_TABLES:
        if entry in table:
            return table[entry]
    raise KeyError(entry)


def selfplay_args(entry: str, **named) -> list:
    """The values of ``named`` in the order ``entry`` takes them (``SELFPLAY_ARGS`` / ``SELFPLAY_ARGS_MORE`` / ``SELFPLAY_ARGS_TABLE``).  A missing or an
    unknown name is a TypeError; nothing is defaulted and nothing converted."""
    names = [name for name, _ in selfplay_table(entry)]
    for name in names:
        if name not in named:
            raise TypeError(f"{entry}: missing argument {name!r}")
    for name in named:
        if name not in names:
            raise TypeError(f"{entry} has no argument {name!r}")
    return [named[name] for name in names]


def selfplay_call(lib, entry: str, **named):
    """``lib.<entry>`` of the self-play family with its arguments given by name."""
    return getattr(lib, entry)(*selfplay_args(entry, **named))


# every symbol include/gobblet_hip.h declares: (name, restype, argtypes)
SIGNATURES = {
    "gbl_layout_info": (_int, [C.POINTER(C.c_int32)]),
    "gbl_last_error": (C.c_char_p, []),
    "gbl_reset": (_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_legal_mask": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "gbl_is_legal": (_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_play_turn": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "gbl_winner": (_int, [_vp, _vp, _i64, _vp]),
    "gbl_flatboard": (_int, [_vp, _vp, _i64, _vp]),
    "gbl_covered": (_int, [_vp, _vp, _i64, _vp]),
    "gbl_validate": (_int, [_vp, _vp, _i64, _vp]),
    "gbl_observe": (_int, [_vp, _vp, _int, _vp, _i64, _vp]),
    "gbl_board_eval": (_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_pinned_alloc": (_int, [_i64, C.POINTER(_vp), C.POINTER(_vp)]),
    "gbl_pinned_free": (_int, [_vp]),
    "gbl_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "gbl_step_into": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "gbl_step_ex": (_int, [_vp] * 14 + [_u64, _u64, _u32, _vp, _i64, _int, _int, _vp]),
    "gbl_sample": (_int, [_vp, _vp, _i64, _u64, _u64, _u32, _vp]),
    "gbl_rollout": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _u64, _u64, _u32, _u32, _int, _vp, _vp, _vp]),
    "gbl_decode_obs": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "gbl_greedy": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _i64, _vp]),
    "gbl_greedy_act": (_int, [_vp, _vp, _vp, _vp, _int, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_sample_at": (_int, [_vp, _vp, _i64, _u64, _u64, _u32, _vp, _vp]),
    "gbl_rollout_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _u64, _u64, _u32, _vp, _u32, _int, _vp, _vp, _vp]),
    "gbl_greedy_act_at": (_int, [_vp, _vp, _vp, _vp, _int, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_playout_values": (_int, [_vp, _vp, _vp, _int, _int, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_tree_search": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_evaluate": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_tree_search_eval": (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gbl_tree_search_eval_noise": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _u64, _u64, _u32] + [_vp] * 8 + [_i64, _vp]),
    "gbl_tree_search_gumbel": (_int, [_vp, _vp, _vp, _vp] + [_int] * 6 + [_u64, _u64, _u32] + [_vp] * 9 + [_i64, _vp]),
    "gbl_solve": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp, _i64, _vp]),
    "gbl_counter_add": (_int, [_vp, _u32, _vp]),
    "gbl_collect": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _u64, _u64, _u32, _vp, _u32,
                           _int, _vp, _vp, _vp]),
    "gbl_collect_from": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _u64, _u64, _u32, _vp, _u32,
                                _int, _vp, _vp, _vp]),
    "gbl_collect_from_ex": (_int, [_vp] * 12 + [_i64, _i64, _i64, _u64, _u64, _u32, _vp, _u32, _int, _vp, _vp, _vp]),
    "gbl_collect_policy": (_int, [_vp] * 14 + [_i64, _i64, _i64, _u64, _u64, _u32, _vp, _u32, _int, _int, _int, _int, _vp, _vp, _vp]),
    **{entry: (_int, [ctype for _, ctype in args]) for table in _SELFPLAY_TABLES for entry, args in table.items()},
    "gbl_outcome_targets": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _u32, _vp]),
    "gbl_symmetry_apply": (_int, [_vp, _int, _vp] + [_vp] * 12 + [_i64, _vp]),
    "gbl_training_batch": (_int, [_vp] * 6 + [_i64, _u32, _i64, _i64, _i64, _int, _u64, _u64, _u32] + [_vp] * 6 + [_vp]),
    "gbl_replay_workspace_bytes": (C.c_size_t, [_i64, _u32]),
    "gbl_replay_append": (_int, [_vp] * 6 + [_i64, _u32, _i64, _i64, C.c_int32] + [_vp] * 3 + [_i64, _vp, _vp, C.c_size_t, _vp]),
    "gbl_replay_batch": (_int, [_vp] * 3 + [_i64, _vp, _i64, _i64, _int, _u64, _u64, _u32] + [_vp] * 6 + [_vp]),
    "gbl_replay_prio_index_bytes": (C.c_size_t, [_i64]),
    "gbl_replay_prio_append": (_int, [_vp] * 4 + [C.c_int32, _i64, _u32, _i64, _i64, _vp, _i64, _vp, _vp, C.c_size_t, _vp]),
    "gbl_replay_prio_update": (_int, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "gbl_replay_prio_index": (_int, [_vp, _i64, _vp, _vp, C.c_size_t, _vp]),
    "gbl_replay_batch_prio": (_int, [_vp] * 3 + [_i64] + [_vp] * 5 + [_i64, _i64, _int, _u64, _u64, _u32] + [_vp] * 6 + [_vp]),
    "gbl_tb_layout": (_int, [_vp, _vp]),
    "gbl_tb_prepare": (_int, [_vp, _vp, _vp]),
    "gbl_tb_sweep": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp]),
    "gbl_tb_index": (_int, [_vp] * 5 + [_i64, _vp]),
    "gbl_tb_position": (_int, [_vp] * 4 + [_i64, _vp]),
    "gbl_tb_probe": (_int, [_vp] * 9 + [_i64, _vp]),
    "gbl_tb_targets": (_int, [_vp] * 4 + [_i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _int, _int] + [_vp] * 3 + [_i64, _vp]),
    "gbl_reanalyse": (_int, [_vp, _int, _int, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64] + [_vp] * 6 + [_i64, _vp]),
    "gbl_reanalyse_gumbel": (_int, [_vp] + [_int] * 6 + [_u64, _u64, _u32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64] + [_vp] * 7 + [_i64, _vp]),
    "gbl_train_workspace_bytes": (_i64, [_i64, _int]),
    "gbl_train_step": (_int, [_vp] * 4 + [_i64, _int] + [_vp] * 7 + [_i64, _vp]),
    "gbl_train_step_weighted": (_int, [_vp] * 4 + [_i64, _int] + [_vp] * 7 + [C.c_float, C.c_int32, C.c_int32] + [_vp] * 3 + [_i64, _vp]),
    "gbl_replay_importance": (_int, [_vp, _i64, C.c_float, _vp, _vp]),
    "gbl_collect_variant": (_int, [_i64, _u32, _int, _int]),
    "gbl_block_alloc": (_int, [_i64, C.POINTER(_vp)]),
    "gbl_block_free": (_int, [_vp]),
    "gbl_device_memory": (_int, [C.POINTER(_i64), C.POINTER(_i64)]),
    "gbl_placement_probe": (_int, [_vp, _i64, _vp, _i64, _i64, _int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), _vp]),
}


class Evaluator(C.Structure):
    """gbl_evaluator (include/gobblet_hip.h): a host struct of four pointers (device pointers for the HIP library) and four ints."""
    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp),
                ("hidden", C.c_int32), ("shift1", C.c_int32), ("shift_p", C.c_int32), ("shift_v", C.c_int32)]


class TrainHyper(C.Structure):
    """gbl_train_hyper (include/gobblet_hip.h): eight floats on the HOST, read when gbl_train_step is called."""
    _fields_ = [(k, C.c_float) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "value_reg", "bias1", "bias2")]


class GobbletHipError(RuntimeError):
    pass


def use_library(path: str) -> None:
    """Load a differently built library of the same ABI instead of csrc/libgobblet_hip.so (kernel A/B experiments, diagnostic
    builds: scripts/, tests/conftest.py).  Call it before anything else of the package touches the library.  The product reads
    no environment variable: the experiment scripts do, and call this."""
    global LIB_PATH, _FOREIGN, _lib
    if _lib is not None:
        raise GobbletHipError("use_library() after the library has been loaded")
    LIB_PATH, _FOREIGN = os.path.abspath(path), True


def needs_build() -> bool:
    if _FOREIGN:
        return not os.path.exists(LIB_PATH)
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > t for s in SOURCES)


def _compiler_env() -> dict:
    """The environment for a compiler child process WITHOUT a profiler's preload: under `rocprofv3 --pmc -- python3
    ...` this process is GPU-initialised by the preloaded tool library, and a child that inherits the preload and
    then execs clang is the exec-after-GPU-init pattern that takes a pool machine down."""
    drop = ("LD_PRELOAD", "HSA_TOOLS_LIB", "HSA_TOOLS_REPORT_LOAD_FAILURE")
    return {k: v for k, v in os.environ.items()
            if k not in drop and not k.startswith(("ROCP", "ROCPROFILER", "ROCTRACER", "ROCTX"))}


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise GobbletHipError("hipcc not found: cannot build csrc/libgobblet_hip.so (there is no CPU fallback)")
    # one builder at a time (ranks of a multi-process launch may all arrive here); the library appears
    # under its final name only when complete
    with open(LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or needs_build():
                tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
                cmd = [hipcc, *HIPCC_FLAGS, "-o", tmp, SOURCES[0]]
                if verbose:
                    print(" ".join(cmd[:-3] + ["-o", LIB_PATH, SOURCES[0]]))
                try:
                    subprocess.check_call(cmd, cwd=CSRC, env=_compiler_env())
                    os.replace(tmp, LIB_PATH)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """The loaded library with typed entry points. Raises if it is missing and cannot be built."""
    global _lib
    if _lib is None:
        path = build()
        try:
            L = C.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise GobbletHipError(f"cannot load {path}: {e} (there is no CPU fallback)") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise GobbletHipError(f"{path} does not export {name}") from e
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        msg = lib().gbl_last_error().decode("utf-8", "replace")
        raise GobbletHipError(f"{what or 'gobblet_hip'} failed (code {rc}): {msg}")


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def device(spec) -> torch.device:
    """``torch.device(spec)`` in the spelling a tensor reports: an unindexed GPU ("cuda") becomes the current one with its index --
    ``torch.device("cuda") != torch.device("cuda:0")``, and every class compares its tensors' devices with its own.  Everything else
    passes through."""
    dev = torch.device(spec)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def current_stream(device):
    """The caller's HIP stream on `device` as a plain pointer (None on the host flavour: its calls are synchronous)."""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return torch.cuda.current_stream(device).cuda_stream


# ---- the HOST flavour of the ABI (include/gobblet_cpu.h, csrc/gobblet_cpu.cpp): gbl_cpu_* -------------------------------------
# A flavour the caller ASKS for (device="cpu": BASELINE config 1 "on CPU", bench.py's CPU twin), never a fallback of the HIP
# path: a "cuda" device without the HIP library still raises.  Built with g++ from the same device header.
CPU_LIB_PATH = os.path.join(CSRC, "libgobblet_cpu.so")
CPU_SOURCES = [os.path.join(CSRC, "gobblet_cpu.cpp"), os.path.join(CSRC, "gobblet_device.h"), os.path.join(CSRC, "gobblet_knobs.h"),
               os.path.join(CSRC, "gobblet_selfplay_entries.inc"), os.path.join(CSRC, "gobblet_env_entries.inc"),
               os.path.join(_HERE, "..", "include", "gobblet_cpu.h"), os.path.join(_HERE, "..", "include", "gobblet_hip.h")]
# -ffp-contract=off: gbl_cpu_train_step's float rule is single IEEE operations (include/gobblet_hip.h); everything else here is integer code
CPU_CXX_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-attributes"] + \
                (["-mpopcnt"] if platform.machine() in ("x86_64", "AMD64") else [])
_NO_HOST_FLAVOUR = ("gbl_pinned_alloc", "gbl_pinned_free", "gbl_block_alloc", "gbl_block_free", "gbl_device_memory",
                    "gbl_placement_probe", "gbl_collect_variant", "gbl_train_workspace_bytes", "gbl_replay_workspace_bytes", "gbl_replay_prio_index_bytes",
                    "gbl_tb_layout")
CPU_SIGNATURES = {"gbl_cpu_" + k[4:]: v for k, v in SIGNATURES.items() if k not in _NO_HOST_FLAVOUR}
CPU_SIGNATURES["gbl_cpu_set_threads"] = (_int, [_int])


def build_cpu(force: bool = False) -> str:
    """Compile the host flavour in-tree (g++; no GPU toolchain needed)."""
    def stale():
        return not os.path.exists(CPU_LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(CPU_LIB_PATH) for s in CPU_SOURCES)
    if not force and not stale():
        return CPU_LIB_PATH
    # (a box with the GPU toolchain but no g++: ROCm's clang++ compiles the host flavour just as well)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("amdclang++") or \
        next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++") if os.path.exists(p)), None)
    if not cxx:
        raise GobbletHipError("no C++ compiler found: cannot build csrc/libgobblet_cpu.so")
    with open(CPU_LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or stale():
                tmp = f"{CPU_LIB_PATH}.{os.getpid()}.tmp"
                try:
                    subprocess.check_call([cxx, *CPU_CXX_FLAGS, "-o", tmp, CPU_SOURCES[0]], cwd=CSRC, env=_compiler_env())
                    os.replace(tmp, CPU_LIB_PATH)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return CPU_LIB_PATH


_cpu_raw = None


def cpu_raw() -> C.CDLL:
    """libgobblet_cpu.so with typed gbl_cpu_* entry points (plain return codes)."""
    global _cpu_raw
    if _cpu_raw is None:
        L = C.CDLL(build_cpu())
        for name, (res, args) in CPU_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _cpu_raw = L
    return _cpu_raw


class _HostFlavour:
    """The host library under the DEVICE entry points' names (``gbl_step`` -> ``gbl_cpu_step``), so that the Python layer above
    is the same code for either flavour.  A failing call raises here, with the host library's own message."""

    def __init__(self, raw):
        self._raw = raw

    def __getattr__(self, name):
        if not name.startswith("gbl_"):
            raise AttributeError(name)
        if name in _NO_HOST_FLAVOUR:
            raise GobbletHipError(f"{name} has no host flavour (device-memory helper)")
        fn = getattr(self._raw, "gbl_cpu_" + name[4:])
        if fn.restype is not _int:
            return fn

        def call(*args):
            rc = fn(*args)
            if rc != OK:
                raise GobbletHipError(f"{name} (host flavour) failed (code {rc}): "
                                      f"{self._raw.gbl_cpu_last_error().decode('utf-8', 'replace')}")
            return rc
        setattr(self, name, call)
        return call


_cpu = None


def lib_for(device):
    """The library that serves `device`: the HIP library for a GPU, the host flavour for "cpu" (asked for, never fallen back to)."""
    global _cpu
    if torch.device(device).type == "cuda":
        return lib()
    if torch.device(device).type != "cpu":
        raise GobbletHipError(f"no flavour of the library serves device {device!r}")
    if _cpu is None:
        _cpu = _HostFlavour(cpu_raw())
    return _cpu
