#!/usr/bin/env python3
"""gbl_train_step on the GPU against the torch eager step it replaces: HIP events, one warm-up, five alternating repetitions.

    python scripts/bench_train_step.py [out.json]      (default: profiles/r17/train_step.json)

Either side runs one Adam step of the 117-H-55 network on the same device tensors, in the same process: GobbletTrainer.step (two
launches) and the body of examples/example_train_evaluator.py's fit_augmented (the forward, the loss, the backward and
torch.optim.Adam).  A repetition is STEPS consecutive steps between two events, reported per step, so that the timed window is not a
single launch gap.  Shapes (B, H): (1 024, 64), (4 096, 64), (4 096, 256), (65 536, 256); batches of about 18 set observation bytes per
row, random candidate sets and visits.  The record also keeps the gradient's distance from float64 autograd per test shape (host
flavour, no GPU needed: tests/test_train_step.py asserts it against torch's float32)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = "cuda:0"
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r17", "train_step.json")
SHAPES = ((1024, 64), (4096, 64), (4096, 256), (65536, 256))
STEPS = 20


def batch_of(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.rand(shape, device=DEV, generator=g)  # noqa: E731
    mask = (rnd(n, 54) < 0.5).to(torch.int8)
    mask[:, 0] = 1
    visits = (torch.randint(0, 200, (n, 54), device=DEV, generator=g) * mask).to(torch.int16)
    visits[:, 0] += 1
    z = torch.randint(-1, 2, (n,), device=DEV, generator=g).to(torch.int8)
    z[::50] = nat.Z_OPEN
    return {"observation": (rnd(n, 117) < 0.15).to(torch.int8), "action_mask": mask, "visits": visits, "z": z}


def torch_stepper(batch, hidden):
    """The eager step of fit_augmented's body on `batch` (a row counts unless its z is open)."""
    l1, l2 = torch.nn.Linear(117, hidden).to(DEV), torch.nn.Linear(hidden, 55).to(DEV)
    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=2e-3, weight_decay=1e-4)

    def step():
        drawn = (batch["z"] != nat.Z_OPEN).float()
        obs, visits, z = batch["observation"].float(), batch["visits"].float(), batch["z"].float() * drawn
        pi = visits / visits.sum(-1, keepdim=True).clamp(min=1)
        out = l2(torch.relu(l1(obs)))
        per = -(pi * torch.log_softmax(out[:, :54], 1)).sum(1) + (out[:, 54].clamp(-1, 1) - z) ** 2 + 1e-2 * out[:, 54] ** 2
        loss = (per * drawn).sum() / drawn.sum().clamp(min=1)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def timed_pair(fns, iters=5, steps=STEPS):
    """{name: [ms per step] * iters} of several callables, one warm-up each, then alternating."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    return times


def stats(ms):
    return {"min_us": 1e3 * min(ms), "median_us": 1e3 * float(np.median(ms)), "max_us": 1e3 * max(ms)}


def device_stepper(batch, hidden):
    trainer = G.GobbletTrainer(hidden=hidden, device=DEV)
    return lambda: trainer.step(batch)


def bench_shape(n, hidden):
    batch = batch_of(n)
    t = timed_pair({"kernel": device_stepper(batch, hidden), "torch": torch_stepper(batch, hidden)})
    row = {"batch": n, "hidden": hidden, "kernel": stats(t["kernel"]), "torch_eager": stats(t["torch"])}
    row["torch_over_kernel"] = row["torch_eager"]["median_us"] / row["kernel"]["median_us"]
    return row


def gradient_rows():
    from tests import test_train_step as T
    cpu = nat.cpu_raw()
    rows = []
    for b, h in T.SHAPES:
        d32, mine = T.gradient_distances(cpu, b, h)
        rows.append({"batch": b, "hidden": h, "torch_float32": d32, "gbl_train_step": mine})
    return rows


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events, one warm-up, five repetitions alternating, %d consecutive steps per repetition, per step" % STEPS,
           "rows": [bench_shape(n, h) for n, h in SHAPES],
           "gradient_distance_from_float64": {"what": "max |g - g64| / max |g64|, host flavour and torch float32 autograd on the CPU",
                                              "rows": gradient_rows()}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
