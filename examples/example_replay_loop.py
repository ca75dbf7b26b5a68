#!/usr/bin/env python3
"""The generation loop with a memory: ONE GobbletTrainer and ONE ReplayBuffer live across the generations.  Generation g collects a
window of self-play with the current evaluator on both sides (one launch), appends its finished plies to the ring under tag = g
(three launches, the oldest rows give way), takes `steps` Adam steps on batches drawn from the whole ring -- or from its newest
`recent` rows -- under random symmetries (three launches per step), and plays the new evaluator against the previous generation's:
    python examples/example_replay_loop.py [device] [--generations G] [--boards N] [--plies T] [--steps S] [--capacity C] [--recent R]
Nothing of a window, the ring or a batch crosses to the host; the same seed gives the same bits on every run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402


def arena(new, old, device, boards, plies, iterations, seed=7):
    """`new` against `old`, half the boards with either colour, each half one launch with auto-reset: (new wins, old wins, finished)."""
    wins, losses, finished = 0, 0, 0
    for nets in ((new, old), (old, new)):
        env = G.BatchedGobblet(max(boards // 2, 1), device, auto_reset=True, seed=seed)
        env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=nets, iterations=iterations), count=True, refresh=False)
        c = env.counters  # (plies, games finished, player_1 wins, player_2 wins)
        w1, w2 = int(c[2]), int(c[3])
        wins, losses, finished = wins + (w1 if nets[0] is new else w2), losses + (w2 if nets[0] is new else w1), finished + int(c[1])
    return wins, losses, finished


def replay_loop(device, generations=4, boards=512, plies=48, steps=200, batch=1024, hidden=64, iterations=64, capacity=65536, recent=None,
                arena_boards=128, noise=0.25):
    """Returns one record per generation: rows in the ring, the last step's losses and the arena score against the generation before."""
    trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
    buf = G.ReplayBuffer(capacity, device)
    ev, log = trainer.evaluator(), []
    for g in range(1, generations + 1):
        env = G.BatchedGobblet(boards, device, auto_reset=True, seed=g, track_turn=True)
        traj = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=iterations, sample_plies=4, noise=noise))
        env.outcome_targets(traj)
        buf.append(env, traj, tag=g)
        stats = buf.fit(trainer, steps, batch=batch, symmetries="all", first_call=(g - 1) * steps, recent=recent)
        new = trainer.evaluator()
        wins, losses, finished = arena(new, ev, device, arena_boards, plies, iterations)
        log.append({"generation": g, "total": buf.total, "size": buf.size, "policy_loss": float(stats[-1, 0]), "value_loss": float(stats[-1, 1]),
                    "arena_wins": wins, "arena_losses": losses, "arena_games": finished,
                    "arena_score": (wins + 0.5 * (finished - wins - losses)) / max(finished, 1)})
        ev = new
    return log


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--generations", type=int, default=4)
    ap.add_argument("--boards", type=int, default=512)
    ap.add_argument("--plies", type=int, default=48)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--recent", type=int, default=None, help="draw from the newest RECENT rows only (default: the whole ring)")
    ap.add_argument("--games", type=int, default=128, help="boards of the arena against the previous generation")
    a = ap.parse_args()
    for r in replay_loop(a.device, a.generations, a.boards, a.plies, a.steps, a.batch, a.hidden, a.iterations, a.capacity, a.recent, a.games):
        print("generation %(generation)d: %(size)d rows in the ring (%(total)d ever appended); policy loss %(policy_loss).3f, value loss "
              "%(value_loss).3f; arena against the generation before: %(arena_wins)d wins, %(arena_losses)d losses of %(arena_games)d "
              "finished games" % r)
