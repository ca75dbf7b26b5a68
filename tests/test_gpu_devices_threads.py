"""The host layer off "cuda:0", off the default stream and off the main thread, on the MI355X (-m gpu): every spelling of the device
through one pipeline of every class, an object whose device is not the current one, two host threads on two streams against the serial
run, the per-thread error text, and every compute entry point without a capture test of its own captured on a side stream and
replayed.  The host flavour is the reference throughout (tests/test_host_threads.py runs the same harness without a GPU)."""
import functools

import pytest
import torch

import gobblet_rl_amd as G
from tests import enqueue_harness as E
from tests import host_contract_harness as H

pytestmark = pytest.mark.gpu
nat = G._native
DEV = "cuda:0"
SPELLINGS = ["cuda", torch.device("cuda"), "cuda:0", torch.device("cuda", 0), 0]


# ---- 1. device spellings ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_pipeline():
    return H.pipeline("cpu")


@functools.lru_cache(maxsize=None)
def cuda0_pipeline():
    return {k: v.cpu() for k, v in H.pipeline(DEV).items()}


def test_pipeline_on_cuda0_equals_the_host_flavour():
    H.same(cuda0_pipeline(), host_pipeline(), "cuda:0 against the host flavour")


@pytest.mark.parametrize("dev", SPELLINGS, ids=repr)
def test_every_spelling_of_the_device(dev):
    got = H.pipeline(dev)
    assert all(v.device == torch.device("cuda", 0) for v in got.values())
    H.same(got, cuda0_pipeline(), "device spelled %r against 'cuda:0'" % (dev,))


@pytest.mark.parametrize("dev", ["cuda", "cuda:0"])
def test_a_host_tensor_is_still_refused(dev):
    """Normalising the device weakens no check: a tensor that does not live on the object's device raises as before."""
    env = G.BatchedGobblet(3, dev, auto_reset=True)
    actions = env.sample_actions()
    with pytest.raises(ValueError):
        env.step(actions, status=torch.zeros(3, dtype=torch.int8))
    with pytest.raises(ValueError):
        env.step(actions, next_actions=torch.zeros(3, dtype=torch.int32))
    batch = {"observation": torch.zeros((2, 117), dtype=torch.int8), "visits": torch.zeros((2, 54), dtype=torch.int16),
             "z": torch.zeros(2, dtype=torch.int8)}
    with pytest.raises(ValueError):
        G.GobbletTrainer(hidden=64, device=dev).step(batch)
    with pytest.raises(ValueError):
        G.Tablebase((1, 0, 0), dev).targets(batch, allow_incomplete=True)
    with pytest.raises(ValueError):
        H.evaluator(dev).reanalyse(batch, iterations=8)
    with pytest.raises(ValueError):
        G.ReplayBuffer(10, dev, prioritized=True).set_priority(torch.zeros((2, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        G.SolverGobbletPolicy(2, device=dev, fallback=G.GreedyGobbletPolicy(2, device="cpu"))


# ---- 2. an object whose device is not the current one -----------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_objects_on_the_second_device_while_the_first_is_current():
    torch.cuda.set_device(0)
    got = H.pipeline(torch.device("cuda", 1))
    assert torch.cuda.current_device() == 0
    assert all(v.device.index == 1 for v in got.values())
    H.same(got, host_pipeline(), "cuda:1 against the host flavour")


class _Launches:
    """A library that notes every entry point called through it."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._log.append(("launch", name))
            return fn(*args)
        return call


def test_the_older_classes_enter_the_device_context_around_every_launch(monkeypatch):
    """BatchedBoard, BatchedGobblet, GreedyGobbletPolicy and RandomAdmissiblePolicy launch inside ``torch.cuda.device(<their device>)``
    (what makes them work while another device is current), pinned here where there is one device only."""
    log = []

    class Recording(torch.cuda.device):
        def __enter__(self):
            log.append(("enter", self.idx))
            return super().__enter__()

        def __exit__(self, *exc):
            log.append(("exit", self.idx))
            return super().__exit__(*exc)
    board = G.BatchedBoard(65, DEV)
    env = G.BatchedGobblet(65, DEV, auto_reset=True, track_turn=True)
    greedy, random = G.GreedyGobbletPolicy(2, device=DEV), G.RandomAdmissiblePolicy(device=DEV)
    monkeypatch.setattr(torch.cuda, "device", Recording)
    for obj in (board, env, env.board, greedy, random):
        obj._lib = _Launches(obj._lib, log)

    def launched(run) -> set:
        """The entry points ``run`` called, each inside the context of device 0."""
        del log[:]
        run()
        inside, names = [], set()
        for what, arg in log:
            if what == "enter":
                inside.append(arg)
            elif what == "exit":
                assert inside.pop() == arg
            else:
                assert inside and inside[-1] == 0, "%s launched outside torch.cuda.device(0)" % arg
                names.add(arg)
        assert not inside
        return names

    def on_board():
        board.is_legal(3, 0); board.legal_mask(0); board.play_turn(0, 3); board.get_flatboard(); board.check_for_winner()
        board.check_covered(); board.evaluate(); board.validate(); board.observation(1)
    assert launched(on_board) == {"gbl_is_legal", "gbl_legal_mask", "gbl_play_turn", "gbl_flatboard", "gbl_winner", "gbl_covered",
                                  "gbl_board_eval", "gbl_validate", "gbl_observe"}

    def on_env():
        env.reset(); env.step(env.sample_actions()); env.rollout(2); env.device_ply(); env.rollout(1); env.advance_ply()
        out = env.trajectory_buffers(2, placement="any")
        env.collect(2, out=out); env.collect(2, policies=("greedy", "random")); env.step_into(env.sample_actions(), out, 0)
        env.step(env.sample_actions(), status=torch.zeros(65, dtype=torch.int8, device=DEV)); env.solve(1); env.refresh()
    assert launched(on_env) >= {"gbl_reset", "gbl_legal_mask", "gbl_observe", "gbl_step", "gbl_sample_at", "gbl_rollout_at", "gbl_counter_add",
                                "gbl_collect_from_ex", "gbl_collect_policy", "gbl_step_ex", "gbl_solve"}

    def on_policies():
        for policy in (greedy, random):
            policy.device_calls()
        greedy.compute_actions(env.observation, env.action_mask); greedy.compute_actions_from_state(env.squares, env.to_move)
        random.compute_actions(env.action_mask)
        greedy.advance_calls(); random.advance_calls()
    assert launched(on_policies) == {"gbl_decode_obs", "gbl_greedy_act_at", "gbl_sample_at", "gbl_counter_add"}
    torch.cuda.synchronize()


# ---- 3. two host threads, two streams ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_workloads():
    return H.workload_a("cpu"), H.workload_b("cpu")


def test_two_threads_on_two_streams_equal_the_serial_run():
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    a, b = H.run_threads([lambda: H.workload_a(DEV), lambda: H.workload_b(DEV)], [lambda s=s: torch.cuda.stream(s) for s in streams])
    torch.cuda.synchronize()
    serial_a, serial_b = H.workload_a(DEV), H.workload_b(DEV)  # fresh objects, the same seeds, the default stream
    torch.cuda.synchronize()
    H.same_rounds(a, serial_a, "self-play, replay and fit: threaded against serial")
    H.same_rounds(b, serial_b, "windows, solver, table and search: threaded against serial")
    H.same_rounds(a, host_workloads()[0], "self-play, replay and fit: against the host flavour")  # (params, m and v are its last entry)
    H.same_rounds(b, host_workloads()[1], "windows, solver, table and search: against the host flavour")


@pytest.mark.parametrize("flavour", ["device", "host"])
def test_error_text_is_per_thread(flavour):
    H.error_text_per_thread(flavour)


def test_gobblet_v1_from_two_threads():
    H.v1_two_threads(DEV)
    H.v1_two_threads("cuda")  # (the same engine and the same lock under either spelling)
    assert len([k for k in G.gobblet_v1._ENGINES if k.startswith("cuda")]) == 1
    assert H.v1_game(DEV, 1) == H.v1_game("cpu", 1)


# ---- 4. "only enqueues on `stream`": every entry point without a capture test of its own -----------------------------------------
@functools.lru_cache(maxsize=None)
def worlds():
    """(the device's world, the host flavour's, and the snapshot each starts every call from): the same bits on both."""
    dev, host = E.world(DEV), E.world("cpu")
    torch.cuda.synchronize()
    return dev, dev.snapshot(), host, host.snapshot()


def test_the_two_worlds_hold_the_same_bits():
    _, dev0, _, host0 = worlds()
    H.same(E.comparable(dev0), E.comparable(host0), "the raw calls' inputs")


@pytest.mark.parametrize("name", E.NAMES)
def test_raw_call_captured_on_a_side_stream(name):
    dev, dev0, host, host0 = worlds()
    outputs = dict((n, o) for n, _, o in E.TABLE)[name]
    host.restore(host0)
    E.run_eager(host, name, nat.lib_for("cpu"), None)
    expected = E.comparable(host.snapshot())
    dev.restore(dev0)
    E.run_eager(dev, name, nat.lib(), nat.current_stream(DEV))  # eager, the default stream
    torch.cuda.synchronize()
    eager = E.comparable(dev.snapshot())
    H.same(eager, expected, name + ": eager against the host flavour")
    start = E.comparable(dev0)
    assert {k for k in eager if not torch.equal(eager[k], start[k])} == set(outputs)
    dev.restore(dev0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):  # (one capture stream: the graph is a chain)
        assert torch.cuda.current_stream().cuda_stream != 0  # (not the default stream, which the eager call used)
        E.run_eager(dev, name, nat.lib(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for replay in range(2):
        dev.restore(dev0)  # the inputs back, the outputs canaries again: a stale replay would show
        torch.cuda.synchronize()
        H.same(E.comparable(dev.snapshot()), start, name + ": restored")
        graph.replay()
        torch.cuda.synchronize()
        H.same(E.comparable(dev.snapshot()), eager, "%s: replay %d against the eager call" % (name, replay))
