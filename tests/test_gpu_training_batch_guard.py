"""Performance guard of gbl_training_batch (-m gpu): the sampler's time per launch at batch 65 536 from the committed record's own
window (65 536 boards x 32 plies of tree-against-tree self-play; profiles/r15/training_batch.json, written by
scripts/bench_training_batch.py) must stay within 15 % of the record's median -- the margin the other guards use; the record's five
repetitions and the box-to-box spread of earlier guards were 8-15 %.  Parity is not checked here: tests/test_gpu_symmetry.py compares
the kernel with the host flavour."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_batch_65536_within_the_record():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_training_batch as B
    with open(os.path.join(ROOT, "profiles", "r15", "training_batch.json")) as f:
        rows = json.load(f)["training_batch"]["rows"]
    record = next(r["kernel"]["median_us"] for r in rows if r["batch"] == 65536)
    env, traj = B.window()
    kernel, _ = B.kernel_launcher(env, traj, 65536)
    us = 1e3 * float(np.median(B.timed_pair({"kernel": kernel})["kernel"]))  # (one warm-up, five repetitions)
    print("gbl_training_batch batch 65536: %.1f us (record %.1f)" % (us, record))
    assert us <= 1.15 * record, (us, record)
