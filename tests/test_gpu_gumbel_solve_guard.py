"""The performance condition of gbl_collect_gumbel_solve on the MI355X (-m gpu): at 4 096 boards, depth 3, 16 plies, Gumbel with 16
iterations, the one launch's median of five may not exceed the median of the composed loop (gbl_solve + gbl_tree_search_gumbel(mask) +
gbl_step_into with a torch pick between them; scripts/bench_selfplay_gumbel_solve.py) measured beside it in the same process, after
both have been seen to play the same games.  The gate is 1.0 x: a condition, not a target -- the record is profiles/r32/
selfplay_gumbel_solve.json, section `guard`."""
import os
import sys

import pytest

from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_launch_no_slower_than_the_composed_loop(G):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_selfplay_gumbel_solve as B
    r = B.GuardedRunner(*B.states(4096), B.seeded_evaluator(B.H), 3, plies=16)
    r.check_equal()
    t = r.time(reps=5, names=("fused", "composed"))
    fused, composed = B.stats(t["fused"]), B.stats(t["composed"])
    print("gbl_collect_gumbel_solve 4096 boards x 16 plies, depth 3: fused %s  composed %s  ratio %.3f"
          % (fused, composed, fused["median"] / composed["median"]))
    assert fused["median"] <= 1.0 * composed["median"], (fused, composed)
