"""Performance guard of gbl_tb_targets (-m gpu): at 65 536 rows on the (1, 1, 2) table, with every optional output NULL but visits_out,
the kernel must not take more than 15 % longer than the two launches it folds, gbl_decode_obs + gbl_tb_probe on the same rows -- both
measured here, in this process, alternating (HIP events, one warm-up, the median of five: scripts/bench_tb_targets.py).  The yardstick
is the existing kernels, not a recorded number of the new one; 15 % is the margin the project's other guards give over the box-to-box
spread.  The new kernel does the same gathers and moves fewer bytes, so parity is the worst case expected.  Parity of the bytes is not
checked here: tests/test_gpu_tb_targets.py compares the kernel with the host flavour."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tb_targets_65536_is_no_slower_than_decode_and_probe():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_tb_targets as P
    t = P.B.timed_pair(P.guard_pair(65536))
    new, old = (1e3 * float(np.median(t[k])) for k in ("gbl_tb_targets", "gbl_decode_obs + gbl_tb_probe"))
    print("65536 rows: gbl_tb_targets %.1f us, gbl_decode_obs + gbl_tb_probe %.1f us" % (new, old))
    assert new <= 1.15 * old, (new, old)
