"""The performance guard of gbl_tree_search_gumbel on the MI355X (-m gpu): 4 096 boards, H = 64, 16 iterations, the Gumbel search
(considered 16, noise on) against the PUCT search (gbl_tree_search_eval), both measured in this process on the same positions."""
import os
import sys

import pytest

from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gumbel_search_no_slower_than_the_puct_search_plus_the_margin(G):
    """The Gumbel median may not exceed the PUCT median by more than 15 %, the project's guard margin for run-to-run spread.  Parity is
    the expectation: both run the same iterations below the root, and at the root the rule replaces three divisions per lane with
    compares; what it adds is one generator block per lane, the considered set once per search and a halving at most once per
    iteration.  The yardstick is the existing kernel measured beside it, not a recorded number."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_gumbel as B
    r = B.SearchRunner(*B.states(4096), B.SMALL, B.seeded_evaluator(B.H))
    t = r.time(reps=5)
    gumbel, puct = B.stats(t["gumbel"]), B.stats(t["eval"])
    print("gumbel %s  puct %s  ratio %.3f" % (gumbel, puct, gumbel["median"] / puct["median"]))
    assert gumbel["median"] <= 1.15 * puct["median"]
