"""Performance guard of gbl_reanalyse_gumbel (-m gpu): at 4 096 rows, H = 64, 16 iterations, the Gumbel form (considered 16, noise on)
must not take more than 15 % longer than gbl_reanalyse at the same 16 iterations -- both measured here, in this process, alternating
(HIP events, one warm-up, the median of five: scripts/bench_reanalyse_gumbel.py).  The margin and the pairing are
tests/test_gpu_gumbel_guard.py's for the single decision, where the same root rule measured 0.91 of the PUCT search: below the root both
run the same iterations, at the root the rule replaces divisions with compares and adds one generator block per lane, the considered
set once per search and a halving at most once per iteration; the read-out adds wave_gumbel_finish and two more butterflies for the
drift.  The yardstick is the existing kernel measured beside it, never a recorded number."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reanalyse_gumbel_4096_is_no_slower_than_reanalyse_plus_the_margin():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_reanalyse_gumbel as P
    fns, keep = P.pair(4096)
    t = P.B.timed_pair({k: fns[k] for k in ("gumbel16", "puct16")})
    new, old = (1e3 * float(np.median(t[k])) for k in ("gumbel16", "puct16"))
    print("4096 rows, 16 iterations: gbl_reanalyse_gumbel %.1f us, gbl_reanalyse %.1f us, ratio %.3f" % (new, old, new / old))
    assert new <= 1.15 * old, (new, old)
