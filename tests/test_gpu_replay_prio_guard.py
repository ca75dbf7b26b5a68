"""Performance guard of the prioritised draw (-m gpu): on a ring of 2^21 slots with random priorities in 1 .. 1 000, at batch 65 536,
the index build plus gbl_replay_batch_prio must not take longer than the composition it replaces on the same device and the same ring --
torch.cumsum of the priorities as int64, torch.searchsorted of 65 536 targets, and gbl_replay_batch standing in for the row gathers.
Both are measured here, in this process, alternating (HIP events, one warm-up, the median of five: scripts/bench_replay_prio.py).  The
ceiling is 1.0 x the composition and no number is fixed in advance: the yardstick is the existing kernel and torch, and a fused draw that
loses to the composition has no reason to exist.  Parity is not checked here: tests/test_gpu_replay_prio.py compares the kernels with
the host flavour."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_and_prioritized_draw_are_no_slower_than_the_torch_composition():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_replay_prio as P
    buf = P.random_ring()
    fused, composed = P.guard_pair(buf)
    print("ring 2^21, batch 65536: index build + gbl_replay_batch_prio %.1f us, cumsum + searchsorted + gbl_replay_batch %.1f us" % (fused, composed))
    assert fused <= 1.0 * composed, (fused, composed)
