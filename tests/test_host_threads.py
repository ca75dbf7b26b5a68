"""The host flavour driven from two threads at once (no GPU needed): two workloads on objects of their own against the serial run of
the same work, the per-thread error text of gbl_cpu_last_error, two gobblet_v1 environments behind one engine, and the device helper
every class normalises its device with.  tests/test_gpu_devices_threads.py runs the same workloads on the MI355X against these."""
import functools

import pytest
import torch

import gobblet_rl_amd as G
from tests import enqueue_harness as E
from tests import host_contract_harness as H

nat = G._native


@functools.lru_cache(maxsize=None)
def serial():
    """Both workloads, one after the other on the main thread (computed once, never changed)."""
    return H.workload_a("cpu"), H.workload_b("cpu")


def test_two_threads_equal_the_serial_run():
    a, b = H.run_threads([lambda: H.workload_a("cpu"), lambda: H.workload_b("cpu")])
    H.same_rounds(a, serial()[0], "self-play, replay and fit")
    H.same_rounds(b, serial()[1], "windows, solver, table and search")
    # (the rounds did something: games ended, rows were stored, the steps counted rows and moved the parameters)
    assert int(serial()[0][-1]["total"][0]) > 300 and float(serial()[0][-2]["fit"][:, 2].min()) > 0
    assert not torch.equal(serial()[0][-1]["params"], G.GobbletTrainer(hidden=64, device="cpu", seed=2).params)


@pytest.mark.parametrize("threads", [1, 3])
def test_the_shared_thread_count_does_not_reach_the_results(threads):
    """gbl_cpu_set_threads is one process-wide number that every caller's workers read: whatever it is while two callers run, the
    results are the serial run's."""
    raw = nat.cpu_raw()
    assert raw.gbl_cpu_set_threads(threads) == nat.OK
    try:
        a, b = H.run_threads([lambda: H.workload_a("cpu", 4), lambda: H.workload_b("cpu", 4)])
    finally:
        assert raw.gbl_cpu_set_threads(0) == nat.OK
    H.same_rounds(a[:4], serial()[0][:4], "self-play, replay and fit")
    H.same_rounds(b, serial()[1][:4], "windows, solver, table and search")


def test_error_text_is_per_thread():
    H.error_text_per_thread("host")


def test_gobblet_v1_from_two_threads():
    H.v1_two_threads("cpu")


def test_device_helper():
    assert nat.device("cpu") == torch.device("cpu") and nat.device(torch.device("cuda", 1)) == torch.device("cuda:1")
    assert nat.device("cuda:3").index == 3 and nat.device("cpu").index is None
    assert torch.device("cuda") != torch.device("cuda:0")  # (why the helper exists)
    for cls in (G.BatchedBoard, G.BatchedGobblet, G.GreedyGobbletPolicy, G.RandomAdmissiblePolicy):
        assert "_OnDevice" in [base.__name__ for base in cls.__mro__]  # (by name: the package can be loaded under two names)


def test_a_tensor_on_another_device_is_still_refused():
    """The checks the normalised device feeds: a tensor that does not live where the object does raises, as before."""
    env = G.BatchedGobblet(3, "cpu", auto_reset=True)
    with pytest.raises(ValueError):
        env.step(torch.zeros(3, dtype=torch.int32), status=torch.zeros(3, dtype=torch.int8, device="meta"))
    with pytest.raises(ValueError):
        G.GobbletTrainer(hidden=64, device="cpu").step({"observation": torch.zeros((2, 117), dtype=torch.int8, device="meta"),
                                                        "visits": torch.zeros((2, 54), dtype=torch.int16), "z": torch.zeros(2, dtype=torch.int8)})


# ---- the raw-call table of tests/enqueue_harness.py on the host flavour: the reference of the capture tests on the device ---------
@functools.lru_cache(maxsize=None)
def host_world():
    w = E.world("cpu")
    return w, w.snapshot()


@pytest.mark.parametrize("name", E.NAMES)
def test_raw_call_changes_its_outputs_and_nothing_else(name):
    w, start = host_world()
    w.restore(start)
    E.run_eager(w, name, nat.lib_for("cpu"), None)
    after = E.comparable(w.snapshot())
    before = E.comparable(start)
    assert {k for k in after if not torch.equal(after[k], before[k])} == set(dict((n, o) for n, _, o in E.TABLE)[name])
    w.restore(start)
    E.run_eager(w, name, nat.lib_for("cpu"), None)
    H.same(E.comparable(w.snapshot()), after, name + ": the same call again")  # (no state between calls)


def test_every_compute_symbol_has_a_capture_test():
    """The table above and the entry points other files capture cover every gbl_* symbol of the binding table but the helpers the
    header's "Conventions" block excludes."""
    compute = {name for name in nat.SIGNATURES if not E.is_helper(name)}
    assert len(set(E.NAMES)) == len(E.NAMES) and not set(E.NAMES) & set(E.ALREADY_CAPTURED)
    assert set(E.NAMES) | set(E.ALREADY_CAPTURED) == compute, sorted(compute ^ (set(E.NAMES) | set(E.ALREADY_CAPTURED)))
