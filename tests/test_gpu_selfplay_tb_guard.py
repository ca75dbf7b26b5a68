"""The performance guard of gbl_collect_search_tb on the MI355X (-m gpu): on the complete (2, 2, 2) table, 4 096 boards x 16 plies of
table against table, the fused launch against the composed loop of existing entry points (gbl_tb_probe + the pick + gbl_step_into
from the same position), both measured in this process."""
import os
import sys

import pytest

from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench(G):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_selfplay_tb as B
    return B, B.full_table()


def test_fused_no_slower_than_the_composed_loop(bench):
    """The fused launch's median against the composed loop's; the margin is the width of the composed loop's own min-max band in
    this run (the rule of tests/test_gpu_selfplay_solve.py's test of the same name)."""
    B, tb = bench
    r = B.Runner(*B.states(4096), tb, "tablebase", plies=16)
    r.check_equal()
    t = r.time(reps=5)
    print("fused %s  composed %s" % (B.stats(t["fused"]), B.stats(t["composed"])))
    assert B.within_spread(t["fused"], t["composed"])
