"""gobblet-rl_amd -- MI355X-native batched Gobblet Gobblers environment.

    BatchedGobblet   lockstep vector env over N boards in HBM (the throughput path)
    BatchedBoard     the reference ``Board`` interface over N boards
    gobblet_v1       ``env() / raw_env()``: the reference's single-env AEC surface over the same engine
    GreedyGobbletPolicy  the reference's depth-1/2 lookahead policy, batched
    MonteCarloGobbletPolicy  flat Monte-Carlo playouts per candidate action (strength tunable by the playout count)
    TreeSearchGobbletPolicy  UCT tree search per board on the same playouts (root visit distribution and values)
    GobbletEvaluator  a small integer network (priors and value of a position) evaluated inside the kernels
    EvaluatorTreeSearchGobbletPolicy  the tree search with that network in place of the playouts
    symmetry         the 512 board symmetries; BatchedGobblet.training_batch draws symmetry-augmented batches on the device
    SolverGobbletPolicy  the exact bounded-depth solver: proven wins and losses per action, optionally over another policy
    GobbletTrainer   the float network behind GobbletEvaluator.from_float and its Adam step on the device (BatchedGobblet.fit)
    ReplayBuffer     a ring of compacted training rows on the device: windows appended, exact symmetry-augmented draws, fit;
                     ReplayBuffer.reanalyse / GobbletEvaluator.reanalyse: stored rows' visits from the current network's search
                     (gumbel=dict(...): the Gumbel root search's target rows, from 16 iterations)
    Tablebase        the game solved outright, one byte per position: retrograde sweeps and probes; TablebaseGobbletPolicy plays from it
                     (BatchedGobblet.collect(search=dict(gumbel=dict(tablebase=tb, judge=True))): the table as a side and as the judge of
                     every ply inside the Gumbel self-play window, one launch)

The compute path is the hand-written HIP library ``csrc/libgobblet_hip.so`` (C-ABI in
``include/gobblet_hip.h``); there is no CPU fallback.  Importing this package needs torch;
using it needs an MI355X.
"""
from . import _native  # noqa: F401
from . import gobblet_v1  # noqa: F401
from . import symmetry  # noqa: F401
from ._native import GobbletHipError, build  # noqa: F401
from .board import BatchedBoard  # noqa: F401
from .vector_env import BatchedGobblet  # noqa: F401
from .greedy_policy import GreedyGobbletPolicy  # noqa: F401
from .playout_policy import MonteCarloGobbletPolicy  # noqa: F401
from .tree_policy import TreeSearchGobbletPolicy  # noqa: F401
from .evaluator_policy import EvaluatorTreeSearchGobbletPolicy, GobbletEvaluator, cap_full, gumbel_row, root_noise  # noqa: F401
from .solver_policy import SolverGobbletPolicy  # noqa: F401
from .trainer import GobbletTrainer  # noqa: F401
from .replay import ReplayBuffer  # noqa: F401
from .tablebase import Tablebase, TablebaseGobbletPolicy  # noqa: F401
from .random_policy import RandomAdmissiblePolicy  # noqa: F401
from .symmetry import N_SYMMETRIES  # noqa: F401
from .sharding import make_shard, reduce_counters, shard_bounds  # noqa: F401

__version__ = "0.1.0"
