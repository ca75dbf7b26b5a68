"""Performance guard of gbl_reanalyse (-m gpu): at 4 096 rows, H = 64, 64 iterations, the fused launch must not take more than 15 %
longer than the composition it replaces -- gbl_decode_obs + gbl_tree_search_eval + the torch narrowing into the int16 rows -- both
measured here, in this process, alternating (HIP events, one warm-up, the median of five: scripts/bench_reanalyse.py).  The yardstick is
the composition measured in this run, never a recorded number of the new kernel; 15 % is the margin the project's other self-measuring
guards give for the run-to-run spread.  Both sides run the same search code (tree_eval_iterations), which dominates, so parity is
what is expected.  Parity of the bytes is checked by the script's own assertion and by tests/test_gpu_reanalyse.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reanalyse_4096_is_no_slower_than_decode_search_and_narrowing():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_reanalyse as P
    fns, keep = P.pair(4096)
    t = P.B.timed_pair(fns)
    new, old = (1e3 * float(np.median(t[k])) for k in ("gbl_reanalyse", "decode_obs + tree_search_eval + torch"))
    print("4096 rows: gbl_reanalyse %.1f us, gbl_decode_obs + gbl_tree_search_eval + narrowing %.1f us" % (new, old))
    assert new <= 1.15 * old, (new, old)
