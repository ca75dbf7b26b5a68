"""What tests/test_host_threads.py and tests/test_gpu_devices_threads.py share: the calling contract of include/gobblet_hip.h's
"Conventions" block -- no state between calls, only enqueue on `stream`, thread-local error text -- exercised through the Python host
layer off "cuda:0", off the default stream and off the main thread.  Every function takes the device, so that the host flavour
("cpu") is the reference of the same run on the GPU.  A plain module: nothing here is collected."""
import contextlib
import json
import os
import threading

import numpy as np
import torch

import gobblet_rl_amd as G

nat = G._native
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JOIN_SECONDS = 300  # a cap, not a measurement: the serial run of either workload takes seconds


def evaluator(dev):
    """Seeded integer weights, H = 64 (as __graft_entry__.smoke draws them), on ``dev``."""
    rng = np.random.default_rng(0)
    return G.GobbletEvaluator(rng.integers(-128, 128, (117, 64), dtype=np.int8), rng.integers(-300, 300, 64),
                              rng.integers(-128, 128, (16, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56), 1, 9, 9, device=dev)


def on(dev, t):
    """A caller-made tensor: built on the host (the same bits for every device), then moved to ``dev`` as the caller spells it."""
    return t.to(dev if not isinstance(dev, int) else torch.device("cuda", dev))


def window(tr):
    return {k: v for k, v in tr.items() if not k.startswith("_")}


def same(got: dict, exp: dict, what: str) -> None:
    """Bit-equal dicts of tensors (compared on the host)."""
    assert set(got) == set(exp), (what, sorted(set(got) ^ set(exp)))
    for k in exp:
        a, b = got[k].cpu(), exp[k].cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        # (floats by their bits: a NaN would equal itself, +0 would differ from -0)
        ai, bi = (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(ai, bi), (what, k, int((ai != bi).sum()))


# ---- part 1 / 2: one short pipeline through every class, on the device as the caller spells it ----------------------------------
def pipeline(dev) -> dict:
    """Every tensor the pipeline returns, by name, still on its device.  20 masked-random plies first, so that games end inside the
    4-ply window and the batches hold real rows."""
    out = {}

    def keep(prefix, d):
        out.update({prefix + "." + k: v.clone() for k, v in d.items() if isinstance(v, torch.Tensor)})
    env = G.BatchedGobblet(130, dev, auto_reset=True, seed=23, track_turn=True)
    env.rollout(20)
    ev = evaluator(dev)
    tr = env.collect(4, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=8, sample_plies=2))
    env.outcome_targets(tr)
    keep("window", window(tr))
    first = env.training_batch(tr, 64, call=0)
    keep("batch0", first)
    batch = env.training_batch(tr, 64, call=1, out=first)
    assert batch is first
    keep("batch1", batch)
    trainer = G.GobbletTrainer(hidden=64, device=dev)
    weights = on(dev, torch.linspace(0.5, 1.5, 64, dtype=torch.float32))
    out["train.stats"] = trainer.step(batch, weights=weights, priority=dict(scale=16.0, floor=1, cap=1000)).clone()
    keep("train", {"params": trainer.params, "m": trainer.m, "v": trainer.v, "row_loss": trainer.last_row_loss,
                   "priority": trainer.last_priority, "hidden_max": trainer.hidden_max})
    buf = G.ReplayBuffer(100, dev, prioritized=True)
    cells = tr["z"].numel()
    buf.append(env, tr, tag=1, priority=on(dev, (torch.arange(cells).reshape(tr["z"].shape) % 5).to(torch.int32)))
    draw = buf.batch(64, call=1, seed=3, prioritized=True)
    keep("draw0", draw)
    w = buf.batch_weights(draw, 0.5)
    out["draw0.weights"] = w.clone()
    buf.set_priority(draw["index"], draw["sym"].to(torch.int32) % 4)
    draw = buf.batch(64, call=2, seed=3, prioritized=True, out=draw)
    keep("draw1", draw)
    assert buf.batch_weights(draw, 0.5, out=w) is w
    out["draw1.weights"], out["replay.priority"] = w.clone(), buf.priority.clone()
    tb = G.Tablebase((1, 1, 1), dev)
    tb.build()
    keep("tablebase", env.tablebase(tb))
    small = tb.position(torch.arange(65, dtype=torch.int64) * (tb.positions // 65))  # (boards the small table does hold)
    keep("tablebase.small", tb.probe(small, torch.zeros(65, dtype=torch.int8)))
    keep("targets", tb.targets({k: v.clone() for k, v in batch.items()}, census=True))
    keep("reanalyse", ev.reanalyse(batch, iterations=8, census=True))
    actions = env.sample_actions().clone()
    status = torch.zeros(130, dtype=torch.int8, device=dev)
    nxt = torch.zeros(130, dtype=torch.int32, device=dev)
    obs, rew, done, win = env.step(actions, status=status, next_actions=nxt)
    keep("step", dict(obs, actions=actions, status=status, next_actions=nxt, rewards=rew, done=done, winner=win, squares=env.squares,
                      to_move=env.to_move, turn=env.turn))
    sym = on(dev, (torch.arange(130) * 37 % nat.SYMMETRIES).to(torch.int16))
    keep("symmetry", G.symmetry.apply(sym, agent=env.to_move, state=env.squares, observation=env.observation,
                                      action_mask=env.action_mask, visits=tr["visits"][3].contiguous(), actions=actions))
    state, to_move = env.squares[:65], env.to_move[:65]
    greedy = G.GreedyGobbletPolicy(2, seed=1, device=dev)
    out["policy.greedy"] = greedy.compute_actions_from_state(state.contiguous(), to_move.contiguous())
    out["policy.greedy.obs"] = G.GreedyGobbletPolicy(2, seed=1, device=dev).compute_actions(env.observation[:65], env.action_mask[:65])
    out["policy.random"] = G.RandomAdmissiblePolicy(seed=1, device=dev).compute_actions(env.action_mask)
    out["policy.playout"] = G.MonteCarloGobbletPolicy(playouts=4, max_plies=16, seed=1, device=dev).compute_actions_from_state(state, to_move)
    tree = G.TreeSearchGobbletPolicy(iterations=8, playouts=2, max_plies=16, seed=1, device=dev)
    out["policy.tree"], out["policy.tree.visits"] = tree.compute_actions_from_state(state, to_move), tree.last_visits
    evp = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=8, device=dev)
    out["policy.evaluator"], out["policy.evaluator.visits"] = evp.compute_actions_from_state(state, to_move), evp.last_visits
    solver = G.SolverGobbletPolicy(2, device=dev, fallback=G.GreedyGobbletPolicy(2, seed=2, device=dev))
    out["policy.solver"], out["policy.solver.outcomes"] = solver.compute_actions_from_state(state, to_move), solver.last_outcomes
    table = G.TablebaseGobbletPolicy(tb, fallback=G.GreedyGobbletPolicy(1, seed=3, device=dev))
    out["policy.table"] = table.compute_actions_from_state(small, torch.zeros(65, dtype=torch.int8))
    board = G.BatchedBoard(65, dev, squares=state)
    out["board.mask"], out["board.winner"] = board.legal_mask(to_move), board.check_for_winner()
    # (not vacuous: the window holds finished games, so the draws found rows and the step counted them)
    assert int((batch["index"][:, 0] >= 0).sum()) > 0 and float(out["train.stats"][2]) > 0
    return out


# ---- part 3: two workloads, each on objects of its own ----------------------------------------------------------------------------
ROUNDS = 20


def workload_a(dev, rounds=ROUNDS) -> list:
    """Evaluator self-play (130 boards, 4 plies, 8 iterations), the outcome targets, a replay append and 2 fit steps at batch 64 per
    round; clones of what every round produced, then the trained parameters and Adam's moments."""
    env = G.BatchedGobblet(130, dev, auto_reset=True, seed=31, track_turn=True)
    ev, trainer, buf = evaluator(dev), G.GobbletTrainer(hidden=64, device=dev, seed=2), G.ReplayBuffer(300, dev)
    kept = []
    for r in range(rounds):
        tr = env.collect(4, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=8, sample_plies=2))
        env.outcome_targets(tr)
        buf.append(env, tr, tag=r)
        stats = buf.fit(trainer, 2, batch=64, first_call=2 * r, seed=7)
        kept.append({**{k: v.clone() for k, v in window(tr).items()}, "fit": stats.clone()})
    kept.append({"params": trainer.params.clone(), "m": trainer.m.clone(), "v": trainer.v.clone(), "total": buf._state.clone()})
    return kept


def workload_b(dev, rounds=ROUNDS) -> list:
    """A greedy-against-random window (gbl_collect_policy), a masked-random window of 4 099 boards x 3 plies (gbl_collect), the depth-2
    solver, a probe of the (1, 1, 1) table and one decision of the evaluator-guided search per round; clones of each."""
    env = G.BatchedGobblet(130, dev, auto_reset=True, seed=37, track_turn=True)
    wide = G.BatchedGobblet(4099, dev, auto_reset=True, seed=41)
    tb = G.Tablebase((1, 1, 1), dev)
    tb.build()
    small = tb.position(torch.arange(65, dtype=torch.int64) * (tb.positions // 65))
    evp = G.EvaluatorTreeSearchGobbletPolicy(evaluator(dev), iterations=8, device=dev)
    kept = []
    for r in range(rounds):
        got = {"greedy." + k: v.clone() for k, v in window(env.collect(3, policies=("greedy", "random"))).items()}
        got.update({"wide." + k: v.clone() for k, v in window(wide.collect(3)).items()})
        got.update({"solve." + k: v for k, v in env.solve(depth=2).items()})
        got.update({"tablebase." + k: v for k, v in env.tablebase(tb).items()})
        got.update({"small." + k: v for k, v in tb.probe(small, torch.full((65,), r % 2, dtype=torch.int8)).items()})
        got["evaluator"] = evp.compute_actions_from_state(env.squares[:65], env.to_move[:65])
        got["evaluator.visits"] = evp.last_visits
        kept.append(got)
    return kept


def run_threads(jobs: list, contexts=None) -> list:
    """``jobs`` (callables) started together, one thread each, job i inside ``contexts[i]()``; the results in order.  A thread's
    exception is re-raised here; a thread still alive after ``JOIN_SECONDS`` fails the test."""
    gate = threading.Barrier(len(jobs))
    results, errors = [None] * len(jobs), []

    def body(i):
        try:
            with (contexts[i]() if contexts else contextlib.nullcontext()):
                gate.wait(JOIN_SECONDS)
                results[i] = jobs[i]()
        except BaseException as e:  # noqa: BLE001  (handed to the main thread)
            errors.append((i, e))
            gate.abort()
    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    if errors:
        raise errors[0][1]
    return results


def same_rounds(got: list, exp: list, what: str) -> None:
    assert len(got) == len(exp)
    for r, (a, b) in enumerate(zip(got, exp)):
        same(a, b, "%s, round %d" % (what, r))


# ---- the error text is per thread -------------------------------------------------------------------------------------------------
def recorded_error(table: str, fn: str, case: str) -> dict:
    """One case of tests/golden/<table>_arg_errors.json.  Only cases the entry point rejects on the host before it launches anything
    are asked for here (n < 0, a missing required pointer): no argument of theirs is ever read."""
    (c,) = [c for c in json.load(open(os.path.join(GOLDEN, table + "_arg_errors.json"))) if c["fn"] == fn and c["case"] == case]
    return c


def error_text_per_thread(flavour: str) -> None:
    """Thread A and thread B each make an argument error of their own, a third thread makes none; after a second barrier each reads
    back its own message and the third reads ""."""
    lib, prefix = {"device": (nat.lib, "gbl_"), "host": (nat.cpu_raw, "gbl_cpu_")}[flavour]
    lib = lib()
    cases = [recorded_error("batch", "symmetry_apply", "n < 0"), recorded_error("replay", "replay_append", "no mask_traj"), None]
    assert cases[0][flavour][1] == "n < 0" and cases[1][flavour][1] == "mask_traj must not be NULL"
    made, read = threading.Barrier(3), {}

    def body(i):
        def run():
            c = cases[i]
            if c is not None:
                assert getattr(lib, prefix + c["fn"])(*c["args"]) == c[flavour][0] == nat.ERR_ARG
            made.wait(JOIN_SECONDS)  # (both errors have been made, on their threads, before anybody reads)
            read[i] = getattr(lib, prefix + "last_error")().decode()
        return run
    run_threads([body(i) for i in range(3)])
    assert read == {0: "n < 0", 1: "mask_traj must not be NULL", 2: ""}


# ---- gobblet_v1: two single-board environments of one device share its engine ---------------------------------------------------
def v1_game(dev, salt: int, plies: int = 40) -> list:
    """``plies`` plies of a ``raw_env`` on ``dev`` with a fixed rule for the moves (a new game where one ends): what every ply saw and
    did, as bytes."""
    env = G.gobblet_v1.raw_env(device=dev)
    env.reset()
    seen = []
    for t in range(plies):
        if all(env.terminations.values()):
            env.reset()
        agent = env.agent_selection
        ob = env.observe(agent)
        legal = np.flatnonzero(ob["action_mask"])
        action = int(legal[(salt + 7 * t) % len(legal)])
        env.step(action)
        seen.append((agent, action, ob["observation"].tobytes(), ob["action_mask"].tobytes(), dict(env.rewards), dict(env.terminations),
                     env.board.squares.tobytes()))
    return seen


def v1_two_threads(dev) -> None:
    got = run_threads([lambda: v1_game(dev, 1), lambda: v1_game(dev, 4)])
    assert got[0] == v1_game(dev, 1) and got[1] == v1_game(dev, 4)
    assert got[0] != got[1] and any(any(s[5].values()) for s in got[0] + got[1])  # (two different games, and games that end)
