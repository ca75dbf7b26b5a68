"""The performance guard of gbl_collect_search_cap on the MI355X (-m gpu): 4 096 boards x 16 plies, H = 64, 64 iterations, noise 64, the
capped window (16 of 64 iterations on a fast ply, share 64 of 256) against the uncapped window (gbl_collect_search_noise), both
measured in this process from the same position."""
import os
import sys

import pytest

from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capped_window_no_slower_than_the_uncapped_one(G):
    """The capped median may not exceed the uncapped one (gate 1.0 x, no margin): a capped ply runs a subset of an uncapped ply's
    iterations plus one generator block, about 0.44 of the evaluations at these settings, and even one lost occupancy step (+45 % at
    worst) leaves 0.44 x 1.45 < 1.  The yardstick is the existing kernel measured beside it, not a recorded number."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_selfplay_cap as B
    r = B.CapRunner(*B.states(4096), B.I, B.seeded_evaluator(B.H), 0, plies=16)
    r.check_same()
    t = r.time(reps=5, names=("noise", "cap16"))
    capped, uncapped = B.stats(t["cap16"]), B.stats(t["noise"])
    print("capped %s  uncapped %s  ratio %.3f" % (capped, uncapped, capped["median"] / uncapped["median"]))
    assert capped["median"] <= uncapped["median"]
