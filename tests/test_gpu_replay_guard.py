"""Performance guard of gbl_replay_batch (-m gpu): at batch 65 536 the draw from the ring that one 65 536-board x 32-ply window of
tree-against-tree self-play was appended to must not take more than 15 % longer than gbl_training_batch's draw from that same window --
both measured here, in this process, alternating (HIP events, one warm-up, the median of five: scripts/bench_replay.py).  The yardstick
is the existing kernel, not a recorded number of the new one; 15 % is the margin the project's other guards give over the run-to-run
spread.  Parity is not checked here: tests/test_gpu_replay.py compares the kernels with the host flavour."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replay_batch_65536_is_no_slower_than_the_window_sampler():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_replay as P
    env, traj = P.B.window()
    buf = P.filled_buffer(env, traj)
    sampler, _ = P.B.kernel_launcher(env, traj, 65536)
    t = P.B.timed_pair({"replay": P.replay_launcher(buf, 65536), "window": sampler})
    replay, window = (1e3 * float(np.median(t[k])) for k in ("replay", "window"))
    print("batch 65536: gbl_replay_batch %.1f us, gbl_training_batch %.1f us" % (replay, window))
    assert replay <= 1.15 * window, (replay, window)
