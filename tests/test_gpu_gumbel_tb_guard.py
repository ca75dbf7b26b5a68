"""The performance guard of gbl_collect_gumbel_tb on the MI355X (-m gpu): on the complete (2, 2, 2) table, 4 096 boards x 16 plies of
a Gumbel-16 side (considered 16) against the table with the judge on, the fused launch against the composed loop of existing entry
points (gbl_tb_probe + gbl_tree_search_gumbel + gbl_sample + the pick + gbl_step_into from the same position;
scripts/bench_selfplay_gumbel_tb.py), both measured in this process after they have been seen to play the same games.  The record is
profiles/r33/selfplay_gumbel_tb.json, section `guard`."""
import os
import sys

import pytest

from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_no_slower_than_the_composed_loop(G):
    """The fused launch's median of five against the composed loop's; the margin is the width of the composed loop's own min-max band
    in this run (the rule of tests/test_gpu_selfplay_tb_guard.py's test of the same name)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_selfplay_gumbel_tb as B
    r = B.TableRunner(*B.states(4096), B.seeded_evaluator(B.H), B.full_table(), plies=16)
    r.check_equal()
    t = r.time(reps=5, names=("fused", "composed"))
    print("gbl_collect_gumbel_tb 4096 boards x 16 plies: fused %s  composed %s" % (B.stats(t["fused"]), B.stats(t["composed"])))
    assert B.within_spread(t["fused"], t["composed"])
