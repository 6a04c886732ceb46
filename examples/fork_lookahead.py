"""One-step look-ahead from a mid-game state: every action tried from the SAME situation, on the device.

    python examples/fork_lookahead.py [GAMES [TICKS [ROLLOUT]]]        (defaults 64, 150, 40)

The reference can only return to a moment of a game by replaying its logged commands from tick 0 (gameplay.hpp:968-986).
Here the policy plays GAMES games of BASELINE configs[1] for TICKS ticks in the first GAMES arenas of a batch of 9 * GAMES;
then

    snap.save(slot_of_arena)                       # game i -> slot i, one launch
    net.memory_rows(True, ...)                     # its agent's recurrent state -> row i, one launch
    snap.load(slot_of_fork)                        # slot i -> arenas 9 i .. 9 i + 8: the fork, one launch
    net.memory_rows(False, ...)                    # row i -> the nine agents

and fork 9 i + k plays action k once (the policy's forward runs as usual, its command is replaced and
update_actions records the action actually played), followed by ROLLOUT ticks of the policy itself.  Printed per game: how
the nine forks' outcomes spread — how many of them the player survived, and the value head's estimate at the end.  Nothing
goes through the host between the first tick and the printed numbers.  The parameters are random: this shows the loop, not a
result."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy

CAP = 2048


def run(games, ticks, rollout, seed=1234):
    arenas = 9 * games
    w = config.baseline_workload("C2", arenas=arenas, auto_reset=0)  # 64 x 64 map, 1 player + 16 zombies, Solo
    assert w.cfg.n_agents == 1
    sim = env.ArenaBatch(w)
    net = policy.PolicyBatch(policy.init_parameters(seed=0), arenas)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sim.set_stream(stream.cuda_stream), net.set_stream(stream.cuda_stream)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        d_keys, d_vals = z((arenas, CAP), torch.int32), z((arenas, CAP), torch.float32)
        d_counts, d_pov = z(arenas, torch.int32), z((arenas, 160), torch.float32)
        d_dense = torch.empty((arenas, 32, 31, 31), dtype=torch.float32, device="cuda")
        d_probs, d_value = z((arenas, 9), torch.float32), z(arenas, torch.float32)
        d_cmd, d_done = z(arenas, torch.uint8), z(arenas, torch.uint8)
        lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
        idx = torch.arange(arenas, dtype=torch.int32, device="cuda")
        slot_of_arena = torch.where(idx < games, idx, torch.full_like(idx, -1))  # game i -> slot i, the rest takes no part
        slot_of_fork = torch.div(idx, 9, rounding_mode="floor").to(torch.int32)   # arena j <- slot j // 9
        forced = (idx % 9).to(torch.int32)                                        # ... and plays action j % 9
        forced_cmd = torch.tensor(list(policy.ACTION_STRING.encode()), dtype=torch.uint8, device="cuda")[forced.long()]
        d_h, d_act = z((games, 2, policy.HIDDEN), torch.float32), z((games, policy.ACTIONS), torch.float32)

        def tick(replace=None):
            sim.observe_sparse_device(*lists)
            sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
            net.predict_sparse(*lists, arenas, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=seed,
                               d_dense_ptr=d_dense.data_ptr())
            if replace is not None:
                d_cmd.copy_(replace[0])
                net.update_actions(replace[1].data_ptr(), arenas)
            sim.step_device(d_cmd.data_ptr(), 1)

        sim.reset(*w.seeds())
        net.reset_memory()
        snap = sim.snapshot(games)
        for _ in range(ticks):
            tick()
        snap.save(slot_of_arena)
        net.memory_rows(True, d_h.data_ptr(), d_act.data_ptr(), slot_of_arena.data_ptr(), games, arenas)
        snap.load(slot_of_fork)
        net.memory_rows(False, d_h.data_ptr(), d_act.data_ptr(), slot_of_fork.data_ptr(), games, arenas)
        tick(replace=(forced_cmd, forced))
        for _ in range(rollout):
            tick()
        sim.observe_sparse_device(*lists)  # the value of where each fork ended up (memory is not needed any more)
        sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
        net.forward_sparse(*lists, arenas, d_probs.data_ptr(), d_value.data_ptr(), d_dense_ptr=d_dense.data_ptr())
        sim.done_device(d_done.data_ptr())
        value = d_value.view(games, 9)
        alive = (1 - d_done.view(games, 9).to(torch.float32))
        rows = torch.stack([alive.sum(1), value.min(1).values, value.max(1).values, value.argmax(1).to(torch.float32)], 1)
        stream.synchronize()
        skipped = snap.status()
        out = rows.cpu().numpy()
        snap.close()
    sim.set_stream(None), net.set_stream(None)
    net.close(), sim.close()
    return out, skipped


if __name__ == "__main__":
    games = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    rollout = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    rows, skipped = run(games, ticks, rollout)
    assert skipped == (0, 0), skipped
    print("%d games forked nine ways at tick %d, %d ticks of rollout behind the forced action" % (games, ticks, rollout))
    print("game  forks alive  value min    value max    best action")
    for i, (alive, lo, hi, best) in enumerate(rows[:16]):
        print("%4d  %11d  %11.6f  %11.6f  %s" % (i, int(alive), lo, hi, policy.ACTION_STRING[int(best)]))
    spread = rows[:, 2] - rows[:, 1]
    print("value spread over the nine forks: mean %.6f, max %.6f; games in which the forced action decided survival: %d of %d"
          % (spread.mean(), spread.max(), int(((rows[:, 0] > 0) & (rows[:, 0] < 9)).sum()), games))
