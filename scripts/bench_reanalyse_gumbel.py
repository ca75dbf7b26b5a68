#!/usr/bin/env python3
"""gbl_reanalyse_gumbel on one MI355X beside gbl_reanalyse, beside the composition it replaces, and gbl_reanalyse of this build beside
a library built from the parent commit -- all in one process, alternating.  HIP events, one warm-up, the median of five with minimum and
maximum (scripts/bench_training_batch.py's timed_pair).  scripts/bench_reanalyse.py's rows and network: the masked-random mix (seed 11,
64 plies), H = 64 seeded integer weights, explore 16; the rule at considered 16, noise on, 50 / 23.  Three parts, each a process of its
own (run each under its own `timeout`, chained with &&); each merges its section into the record:

    python scripts/bench_reanalyse_gumbel.py kernel [out.json] [--parent lib.so]
        4 096 and 65 536 rows, a batch's pitches, visits and drift out:
        parent   gbl_reanalyse of this build against the parent's at 16 and 64 iterations (the same instantiation: this build's median
                 must lie inside the parent's min-max band; without --parent the comparison is recorded as NOT MEASURED)
        gumbel   gbl_reanalyse_gumbel at 16 iterations against gbl_reanalyse at 64 and at 16, and against gbl_decode_obs +
                 gbl_tree_search_gumbel + the torch narrowing of the target bytes into the int16 rows
    python scripts/bench_reanalyse_gumbel.py ring [out.json]     a ring of 2^20 live rows refreshed in place, the Gumbel form at 16
                                                                 iterations against the PUCT form at 64
    python scripts/bench_reanalyse_gumbel.py fit [out.json]      one step of ReplayBuffer.fit at batch 1 024: plain, reanalyse= at 64
                                                                 PUCT iterations, reanalyse=dict(gumbel=...) at 16
    python scripts/bench_reanalyse_gumbel.py --host [out.json]   one seed of examples/example_reanalyse_gumbel.py on the host flavour

Default record: profiles/r30/reanalyse_gumbel.json.  Recorded numbers, no gate (tests/test_gpu_reanalyse_gumbel_guard.py asserts its own
ratio)."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import bench_reanalyse as P  # noqa: E402  (the rows, the network, the ring)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

B, BS, DEV = P.B, P.BS, P.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r30", "reanalyse_gumbel.json")
SMALL, LARGE, EXPLORE = 16, 64, P.EXPLORE
CONSIDERED, OFFSET, SCALE = 16, 50, 23
RULE = dict(considered=CONSIDERED, noise=True, visit_offset=OFFSET, scale=SCALE)


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_reanalyse", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


def launchers(ev, n, obs, mask, visits, parent=None):
    """Callables on the same n dense rows (visits: the int16 (n, 54) destination, in place)."""
    lib, s = nat.lib(), nat.current_stream(DEV)
    struct = ev.as_struct()
    moved = torch.empty(n, dtype=torch.int32, device=DEV)
    state, who = torch.empty((n, nat.CELLS), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    target = torch.empty((n, nat.ACTIONS), dtype=torch.uint8, device=DEV)
    call = [0]

    def puct(iterations, L=lib, name="gbl_reanalyse"):
        def run():
            rc = L.gbl_reanalyse(C.addressof(struct), iterations, EXPLORE, obs.data_ptr(), nat.OBS_BYTES, mask.data_ptr(), nat.ACTIONS, visits.data_ptr(),
                                 visits.data_ptr(), nat.ACTIONS, None, 1, None, None, None, None, moved.data_ptr(), None, n, s)
            assert rc == 0, (name, L.gbl_last_error())
        return run

    def gumbel():
        call[0] += 1
        nat.check(lib.gbl_reanalyse_gumbel(C.addressof(struct), SMALL, EXPLORE, CONSIDERED, 1, OFFSET, SCALE, 0, 0, call[0], obs.data_ptr(),
                                           nat.OBS_BYTES, mask.data_ptr(), nat.ACTIONS, visits.data_ptr(), visits.data_ptr(), nat.ACTIONS, None, 1,
                                           None, None, None, None, moved.data_ptr(), None, None, n, s), "gbl_reanalyse_gumbel")

    def composition():
        call[0] += 1
        nat.check(lib.gbl_decode_obs(obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, s), "gbl_decode_obs")
        nat.check(lib.gbl_tree_search_gumbel(state.data_ptr(), who.data_ptr(), mask.data_ptr(), C.addressof(struct), SMALL, EXPLORE, CONSIDERED, 1,
                                             OFFSET, SCALE, 0, 0, call[0], None, None, None, None, None, None, None, target.data_ptr(), None, n, s),
                  "gbl_tree_search_gumbel")
        visits.copy_(target)  # (the widening into the int16 rows; no drift)

    fns = {"gumbel16": gumbel, "puct16": puct(SMALL), "puct64": puct(LARGE), "decode_obs + tree_search_gumbel + torch": composition}
    if parent is not None:
        fns["parent_puct16"], fns["parent_puct64"] = puct(SMALL, parent, "parent"), puct(LARGE, parent, "parent")
    return fns, call


def pair(n, parent=None):
    """The callables at n rows of the mix with a batch's pitches, the fused launch checked against the composition once."""
    ev = P.evaluator()
    obs, mask = P.mix_rows(n)
    visits = torch.zeros((n, nat.ACTIONS), dtype=torch.int16, device=DEV)
    fns, call = launchers(ev, n, obs, mask, visits, parent)
    fns["gumbel16"]()
    mine = visits.clone()
    call[0] -= 1                                   # (the same call number: the same noise)
    fns["decode_obs + tree_search_gumbel + torch"]()
    torch.cuda.synchronize()
    assert torch.equal(mine, visits), "the kernel and the composition disagree"
    return fns, (ev, obs, mask, visits)


def inside(ms, band):
    m = sorted(ms)[len(ms) // 2]
    return min(band) <= m <= max(band)


def kernel(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    rows = []
    for n in (4096, 65536):
        fns, keep = pair(n, parent)
        t = B.timed_pair(fns)
        s = {k: B.stats(v) for k, v in t.items()}
        g = s["gumbel16"]["median_us"]
        row = {"rows": n, **s, "gumbel16_over_puct64": g / s["puct64"]["median_us"], "gumbel16_over_puct16": g / s["puct16"]["median_us"],
               "gumbel16_over_composition": g / s["decode_obs + tree_search_gumbel + torch"]["median_us"]}
        if parent is not None:
            for its in (SMALL, LARGE):
                row["puct%d_inside_parent_band" % its] = inside(t["puct%d" % its], t["parent_puct%d" % its])
                row["puct%d_over_parent" % its] = s["puct%d" % its]["median_us"] / s["parent_puct%d" % its]["median_us"]
        else:
            row["parent"] = "NOT MEASURED"
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fns, keep
        torch.cuda.empty_cache()
    BS.merge(path, "kernel", {"device": torch.cuda.get_device_name(0), "hidden": P.HIDDEN, "explore": EXPLORE, "gumbel": RULE, "rows": rows})


def ring(path):
    ev, buf = P.evaluator(), P.selfplay_ring(1 << 20)
    assert buf.size == 1 << 20
    call = [0]

    def gumbel():
        call[0] += 1
        buf.reanalyse(ev, SMALL, EXPLORE, gumbel=RULE, call=call[0])
    t = B.timed_pair({"ReplayBuffer.reanalyse, gumbel 16": gumbel, "ReplayBuffer.reanalyse, puct 64": lambda: buf.reanalyse(ev, LARGE, EXPLORE)})
    s = {k: B.stats(v) for k, v in t.items()}
    rec = {"ring_rows": buf.size, **s, "gumbel16_over_puct64": s["ReplayBuffer.reanalyse, gumbel 16"]["median_us"] / s["ReplayBuffer.reanalyse, puct 64"]["median_us"]}
    print(json.dumps(rec), flush=True)
    BS.merge(path, "ring_in_place", rec)


def fit(path):
    ev, buf = P.evaluator(), P.selfplay_ring(1 << 20)
    a, b, c = (G.GobbletTrainer(hidden=64, device=DEV, seed=0) for _ in range(3))
    step = [0]

    def gumbel():
        step[0] += 1
        buf.fit(c, 1, batch=1024, first_call=step[0], reanalyse=dict(evaluator=ev, iterations=SMALL, explore=EXPLORE, gumbel=RULE))
    t = B.timed_pair({"fit step, plain": lambda: buf.fit(a, 1, batch=1024),
                      "fit step, reanalyse= puct 64": lambda: buf.fit(b, 1, batch=1024, reanalyse=dict(evaluator=ev, iterations=LARGE, explore=EXPLORE)),
                      "fit step, reanalyse= gumbel 16": gumbel})
    rec = {"batch": 1024, "hidden": 64, **{k: B.stats(v) for k, v in t.items()}}
    print(json.dumps(rec), flush=True)
    BS.merge(path, "fit_step", rec)


def host(path):
    import example_reanalyse_gumbel as EX
    rec = EX.refresh("cpu", boards=256, plies=24, steps=50, batch=1024)
    rec["note"] = "one seed of examples/example_reanalyse_gumbel.py on the host flavour; whether the refreshed targets train a better network is NOT MEASURED"
    print(json.dumps(rec), flush=True)
    BS.merge(path, "example_host_flavour", rec)


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = args[i + 1]
        del args[i:i + 2]
    if "--host" in args:
        args.remove("--host")
        return host(args[0] if args else DEFAULT_OUT)
    part, path = args[0], (args[1] if len(args) > 1 else DEFAULT_OUT)
    if part == "kernel":
        kernel(path, parent)
    else:
        {"ring": ring, "fit": fit}[part](path)


if __name__ == "__main__":
    main()
