"""Performance guard of gbl_train_step_weighted (-m gpu): at batch 4 096, H = 64 the weighted step -- weights, row_loss_out and prio_out
all given -- must stay within 15 % (the project's guard margin) of gbl_train_step measured in the same process: HIP events, one
warm-up, the median of five alternating repetitions of 20 steps (scripts/bench_train_step.py's batch and timing loop).  Parity is not
checked here: tests/test_gpu_train_weighted.py compares the kernels with the host flavour."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weighted_step_4096_64_within_the_unweighted_step():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_train_step as B
    import bench_train_weighted as BW
    batch = B.batch_of(4096)
    t = B.timed_pair({"plain": B.device_stepper(batch, 64), "weighted": BW.weighted_stepper(batch, 64)})   # (one warm-up, five repetitions)
    plain, weighted = (1e3 * float(np.median(t[k])) for k in ("plain", "weighted"))
    print("batch 4096, H 64: gbl_train_step %.1f us, gbl_train_step_weighted %.1f us per step" % (plain, weighted))
    assert weighted <= 1.15 * plain, (weighted, plain)
