#!/usr/bin/env python3
"""gbl_train_step_weighted, gbl_replay_importance and the loss-driven fit step on the GPU: HIP events, one warm-up, five alternating
repetitions of 20 consecutive calls (scripts/bench_train_step.py's method), median [min, max] in microseconds per call.

    python scripts/bench_train_weighted.py [out.json]                  (default: profiles/r26/train_weighted.json, merged into)
    python scripts/bench_train_weighted.py --tree DIR out.json         the prioritised fit step of ANOTHER checkout (the parent commit's,
                                                                       built in DIR), with that checkout's package: "parent_fit_step"
    GOBBLET_HIP_LIB=build/lib_one_group.so python scripts/bench_train_weighted.py --importance-only out.json
                                                                       gbl_replay_importance of an experiment build
                                                                       (scripts/build_variant.sh one_group -DGBL_IMPORTANCE_ONE_GROUP=1)

(a) the weighted step -- weights, row_loss_out and prio_out all given -- against gbl_train_step at the four (B, H) shapes of 5.16 and
    at (4 096, 192), the one hidden size at which the weighted kernel holds fewer wavefronts per SIMD (--steps-only: this part alone);
(b) gbl_replay_importance at batch 1 024 and 65 536 (the product's grid form; the one-workgroup form through the experiment build);
(c) a full loss-driven fit step (nine launches: fit(prioritized=True, beta=, priority=)) against the prioritised fit step as it was
    (fit(prioritized=True)), H = 64, batch 4 096, on scripts/bench_replay_prio.py's full ring of 2^21 slots."""
import json
import os
import sys

import numpy as np
import torch

ARGS = sys.argv[1:]
TREE = ARGS[ARGS.index("--tree") + 1] if "--tree" in ARGS else None
ROOT = os.path.abspath(TREE) if TREE else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gobblet_rl_amd as G  # noqa: E402
if os.environ.get("GOBBLET_HIP_LIB"):  # an experiment's own build of the library (scripts/build_variant.sh)
    G._native.use_library(os.environ["GOBBLET_HIP_LIB"])
import bench_train_step as B  # noqa: E402  (the timing and the batches)

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r26", "train_weighted.json")
PRIORITY = dict(scale=1000, floor=1, cap=100000)
FIT_BATCH, SLOTS = 4096, 1 << 21


def weighted_stepper(batch, hidden):
    """GobbletTrainer.step with weights in (0, 1] and a priority map: gbl_train_step_weighted with all three optional arrays."""
    trainer = G.GobbletTrainer(hidden=hidden, device=DEV)
    n = batch["z"].shape[0]
    weights = 1.0 - torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    return lambda: trainer.step(batch, weights=weights, priority=PRIORITY)


def bench_steps():
    rows = []
    for n, h in B.SHAPES + ((4096, 192),):
        batch = B.batch_of(n)
        t = B.timed_pair({"plain": B.device_stepper(batch, h), "weighted": weighted_stepper(batch, h)})
        row = {"batch": n, "hidden": h, "gbl_train_step": B.stats(t["plain"]), "gbl_train_step_weighted": B.stats(t["weighted"])}
        row["weighted_over_plain"] = row["gbl_train_step_weighted"]["median_us"] / row["gbl_train_step"]["median_us"]
        rows.append(row)
    return rows


def bench_importance():
    lib, out = G._native.lib(), {}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for n in (1024, 65536):
        prio = torch.randint(1, 100001, (n,), device=DEV, dtype=torch.int32)
        w = torch.empty(n, dtype=torch.float32, device=DEV)
        fn = lambda: G._native.check(lib.gbl_replay_importance(prio.data_ptr(), n, 0.5, w.data_ptr(), stream))  # noqa: E731
        out["batch %d" % n] = B.stats(B.timed_pair({"importance": fn})["importance"])
    return out


def bench_fit(loss_driven=True):
    import bench_replay_prio as P
    buf = P.random_ring(SLOTS)
    names = ("prioritized", "loss_driven") if loss_driven else ("prioritized",)
    trainers = {k: G.GobbletTrainer(hidden=64, device=DEV, seed=1) for k in names}
    call = [0]

    def step(name):
        extra = dict(beta=0.5, priority=PRIORITY) if name == "loss_driven" else {}

        def fn():
            call[0] += 1
            buf.fit(trainers[name], 1, batch=FIT_BATCH, first_call=call[0], prioritized=True, **extra)
        return fn
    t = B.timed_pair({k: step(k) for k in names})
    return {"batch": FIT_BATCH, "hidden": 64, "slots": SLOTS, **{k: B.stats(v) for k, v in t.items()}}


def main():
    rest = [a for i, a in enumerate(ARGS) if not a.startswith("--") and (i == 0 or ARGS[i - 1] != "--tree")]
    path = rest[0] if rest else DEFAULT_OUT
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec["device"] = torch.cuda.get_device_name(0)
    rec["timing"] = "HIP events, one warm-up, five repetitions alternating, %d consecutive calls per repetition, per call" % B.STEPS
    if TREE:
        rec["parent_fit_step"] = bench_fit(loss_driven=False)
    elif "--importance-only" in ARGS:
        rec["importance_" + os.path.basename(os.environ.get("GOBBLET_HIP_LIB", "product"))] = bench_importance()
    elif "--steps-only" in ARGS:
        rec["steps"] = bench_steps()
    else:
        rec["steps"] = bench_steps()
        rec["importance_grid"] = bench_importance()
        rec["fit_step"] = bench_fit()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
