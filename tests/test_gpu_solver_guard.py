"""Performance guard of gbl_solve (-m gpu): k_solve's time per launch on the committed record's own boards must stay within 15 % of
the record (profiles/r14/solver.json, written by scripts/bench_solver.py; the margin the other guards use).  The guarded row is
4 096 boards at depth 4, ~50 ms a launch, whose five repetitions in the record spread by 0.2 %; depth 3 is ~1 ms a launch and its
record spreads by several per cent at 65 536 boards, too close to the margin for a guard.  Parity is not checked here:
tests/test_gpu_solver.py compares the kernel with the host flavour."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("depth", [4])
def test_solve_4096_boards_within_the_record(depth):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_solver
    from tests.search_harness import DEV, Call
    with open(os.path.join(ROOT, "profiles", "r14", "solver.json")) as f:
        rows = json.load(f)["timing_libgobblet_hip.so"]
    record = next(r["device"]["median_ms"] for r in rows if r["boards"] == 4096 and r["depth"] == depth)
    n = 4096
    launch = Call("solve", DEV).load(*(t.cpu().numpy() for t in bench_solver.states(n))).launch

    def go():
        launch((depth,))
    ms = bench_solver.timed(go, iters=3)["median_ms"]  # (one warm-up, three repetitions)
    print("gbl_solve 4096 boards depth %d: %.4f ms (record %.4f)" % (depth, ms, record))
    assert ms <= 1.15 * record, (ms, record)
