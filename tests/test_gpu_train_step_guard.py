"""Performance guard of gbl_train_step (-m gpu): one Adam step at batch 4 096, H = 64 must stay within 15 % of the committed record's
median (profiles/r17/train_step.json, written by scripts/bench_train_step.py, whose batch and timing loop this test runs) -- the margin
the other guards use.  Parity is not checked here: tests/test_gpu_train_step.py compares the kernels with the host flavour."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_step_4096_64_within_the_record():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_train_step as B
    with open(os.path.join(ROOT, "profiles", "r17", "train_step.json")) as f:
        rows = json.load(f)["rows"]
    record = next(r["kernel"]["median_us"] for r in rows if (r["batch"], r["hidden"]) == (4096, 64))
    us = 1e3 * float(np.median(B.timed_pair({"kernel": B.device_stepper(B.batch_of(4096), 64)})["kernel"]))  # (one warm-up, five repetitions)
    print("gbl_train_step batch 4096, H 64: %.1f us per step (record %.1f)" % (us, record))
    assert us <= 1.15 * record, (us, record)
