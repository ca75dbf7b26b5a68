"""Board symmetries (include/gobblet_hip.h, "Board symmetries"): the 8 symmetries of the square times the exchange of the two
equal-sized pieces of a colour, 512 elements, and their action on every row type the library moves.

A symmetry is an integer ``s`` in [0, 512): bits 0-1 = rot, bit 2 = flip (flip first: c <- 2 - c; then rot times (r, c) <- (c, 2 - r)),
bits 3-5 swap player_1's pieces 2k+1 <-> 2k+2, bits 6-8 player_2's.  ``position_map`` / ``action_map`` restate the two maps in Python
(they are what ``compose`` and ``inverse`` are built from); ``apply`` is one launch of ``gbl_symmetry_apply`` (the host flavour for
tensors on the CPU).  The square's symmetries commute with the rules except for ``check_for_winner`` on boards where both colours
hold a line at once, where the reference's "last matching line decides" makes the order of the lines count; the piece swaps are
exact everywhere."""
from __future__ import annotations

import contextlib

import torch

from . import _native as nat

N_SYMMETRIES = nat.SYMMETRIES


def _code(s) -> int:
    s = int(s)
    if not 0 <= s < N_SYMMETRIES:
        raise ValueError("a symmetry is an integer in [0, 512)")
    return s


def position_map(s) -> list:
    """sigma: ``position_map(s)[p]`` is the position a piece on p moves to."""
    s = _code(s)
    out = []
    for p in range(9):
        r, c = divmod(p, 3)
        if s & 4:
            c = 2 - c
        for _ in range(s & 3):
            r, c = c, 2 - r
        out.append(3 * r + c)
    return out


def piece_map(s, agent) -> list:
    """tau_agent: ``piece_map(s, agent)[piece]`` for piece 1..6 (entry 0 is 0)."""
    bits = (_code(s) >> (6 if int(agent) else 3)) & 7
    return [0] + [((q - 1) ^ ((bits >> ((q - 1) // 2)) & 1)) + 1 for q in range(1, 7)]


def action_map(s, agent) -> list:
    """A_agent: ``action_map(s, agent)[a]`` is the image of action a = 9 (piece - 1) + p of that agent."""
    sigma, tau = position_map(s), piece_map(s, agent)
    return [9 * (tau[a // 9 + 1] - 1) + sigma[a % 9] for a in range(nat.ACTIONS)]


def _maps(s):
    return tuple(position_map(s)), tuple(piece_map(s, 0)), tuple(piece_map(s, 1))


_BY_MAPS = {}


def _from_maps(maps) -> int:
    if not _BY_MAPS:
        _BY_MAPS.update({_maps(s): s for s in range(N_SYMMETRIES)})
    return _BY_MAPS[maps]


def compose(g, h) -> int:
    """The symmetry "apply h, then g"."""
    (sg, t0g, t1g), (sh, t0h, t1h) = _maps(g), _maps(h)
    return _from_maps((tuple(sg[sh[p]] for p in range(9)), tuple(t0g[t0h[q]] for q in range(7)), tuple(t1g[t1h[q]] for q in range(7))))


def inverse(g) -> int:
    sg, t0, t1 = _maps(g)
    inv = [0] * 9
    for p, q in enumerate(sg):
        inv[q] = p
    return _from_maps((tuple(inv), t0, t1))  # (a swap is its own inverse)


def apply(sym, agent=None, state=None, observation=None, action_mask=None, visits=None, priors=None, actions=None) -> dict:
    """The images of the given rows under ``sym`` -- an int for every board, or an integer tensor (n,) with one code per board -- as
    new tensors on the rows' device, in ONE launch: ``state`` int8 (n, 27), ``observation`` int8 (n, 3, 3, 13) or (n, 117),
    ``action_mask`` int8 (n, 54), ``visits`` int16 (n, 54), ``priors`` uint8 (n, 54), ``actions`` int32 (n,).  ``agent`` int8 (n,):
    whose view / whose actions each board's rows are (needed for everything but ``state``)."""
    rows = {"state": (state, torch.int8, (nat.CELLS,)), "observation": (observation, torch.int8, None),
            "action_mask": (action_mask, torch.int8, (nat.ACTIONS,)), "visits": (visits, torch.int16, (nat.ACTIONS,)),
            "priors": (priors, torch.uint8, (nat.ACTIONS,)), "actions": (actions, torch.int32, ())}
    given = {k: v for k, v in rows.items() if v[0] is not None}
    if not given:
        raise ValueError("apply: no rows given")
    first = next(iter(given.values()))[0]
    device, n = nat.device(first.device), first.shape[0]
    ins = {}
    for k, (t, dtype, tail) in given.items():
        if k == "observation":
            tail = tuple(t.shape[1:])
            if tail not in ((3, 3, 13), (nat.OBS_BYTES,)):
                raise ValueError("observation: (n, 3, 3, 13) or (n, 117)")
        if t.dtype != dtype or t.device != device or tuple(t.shape) != (n,) + tail:
            raise ValueError(f"{k}: {dtype} {(n,) + tail} on {device}")
        ins[k] = t.contiguous()
    if agent is None and set(ins) != {"state"}:
        raise ValueError("apply: agent (int8 (n,)) is needed for everything but state")
    if agent is not None:
        if agent.dtype != torch.int8 or agent.device != device or tuple(agent.shape) != (n,):
            raise ValueError(f"agent: int8 ({n},) on {device}")
        agent = agent.contiguous()
    if isinstance(sym, torch.Tensor):
        if tuple(sym.shape) != (n,) or sym.is_floating_point():
            raise ValueError(f"sym: an int, or an integer tensor ({n},)")
        codes, sym_all = sym.to(device=device, dtype=torch.int16).contiguous(), 0
    else:
        codes, sym_all = None, _code(sym)
    outs = {k: torch.empty_like(t) for k, t in ins.items()}
    pairs = []
    for k in ("state", "observation", "action_mask", "visits", "priors", "actions"):
        pairs += [nat.ptr(ins.get(k)), nat.ptr(outs.get(k))]
    lib = nat.lib_for(device)
    with torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext():
        nat.check(lib.gbl_symmetry_apply(nat.ptr(codes), sym_all, nat.ptr(agent), *pairs, n, nat.current_stream(device)),
                  "gbl_symmetry_apply")
    return outs
