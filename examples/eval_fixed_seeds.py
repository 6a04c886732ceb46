"""Fixed-seed evaluation with per-arena restarts: no arena waits for the longest game of the batch.

    python examples/eval_fixed_seeds.py ARENAS GAMES [MAX_STEPS [RESTART_EVERY]]

The reference starts every new game with a fresh setup() and a new `tb` as soon as the one before is over
(gameplay.hpp:1231-1277).  With auto_reset = 0 — what a fixed-seed evaluation wants: the caller names every seed — a batch
used to stand still until its longest game had ended and the whole batch was reset.  Here every arena plays the games of a
seed list that lives on the device, one after the other: each tick

    sim.reset_arenas(done=True, max_steps=MAX_STEPS, tb_ptr=.., serial_ptr=.., selected_ptr=..)   # finished or too long: next seed
    net.reset_memory(selected)                                                                  # a new game, a fresh Agent
    observe -> predict -> step

with no host synchronisation inside the loop: which arena takes which seed next is kept by a few tensor operations on
the same stream.  The loop runs GAMES x MAX_STEPS ticks, so every arena plays at least GAMES games (its seed list is GAMES
long and is taken round and round); games that ended are read from the episode log at the end, games cut by the step
limit are the restarts that followed no finished game (a cut game is no episode; the restarts are counted on the device).  The policy's parameters are random: this shows the loop, not
a result.

What a restart costs: a restarted arena runs _srand's 1024 warm-up draws (random.hpp:64-76) in its one wavefront, about
0.3 ms on an MI355X however few arenas restart, and the launch sits in the stream in front of the tick (DESIGN.md §4 has the
figures; auto_reset hides those draws by spreading them over the steps of the game before, which needs the next seed to be
known in advance).  With thousands of arenas some game ends at almost every tick, so a tick of 0.15 ms pays for it almost
every time.  RESTART_EVERY = n makes the call every n-th tick only: a finished arena then waits up to n - 1 ticks and a
game may run up to n - 1 steps past MAX_STEPS, and the cost is shared by n ticks.

run(.., whole_batch=True) is the old way for comparison — GAMES rounds of sf_reset + MAX_STEPS ticks, finished
arenas standing still — which tools/reset_sel_time.py times against this one.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import torch

from strikeforce_amd import config, env, policy

CAP = 2048


def run(arenas, games, max_steps, whole_batch=False, restart_every=1):
    """Returns a dict: ticks, games finished, games cut, live agent-steps (ticks of arenas whose game was running), seconds."""
    w = config.baseline_workload("C2", arenas=arenas, auto_reset=0)  # 64x64 map, 1 player + 16 zombies, Solo
    sim = env.ArenaBatch(w)
    agents = arenas * w.cfg.n_agents
    net = policy.PolicyBatch(policy.init_parameters(seed=0), agents)
    stream = torch.cuda.Stream()
    finished = cut_host = 0
    with torch.cuda.stream(stream):
        sim.set_stream(stream.cuda_stream), net.set_stream(stream.cuda_stream)
        sim.enable_episode_log(64)
        # the seed list: game g of arena a runs on tb = 1 700 000 000 + g * arenas + a (SURVEY §8d's seeds, one block per game)
        a_idx = torch.arange(arenas, dtype=torch.int64, device="cuda")
        seed_list = 1_700_000_000 + torch.arange(games, dtype=torch.int64, device="cuda")[:, None] * arenas + a_idx[None, :]
        d_serial = torch.full((arenas,), 123_456_789, dtype=torch.int64, device="cuda")
        d_tb = seed_list[1 % games].clone()               # what each arena takes at its next restart
        game = torch.ones(arenas, dtype=torch.int64, device="cuda")  # games started per arena
        d_sel = torch.zeros((arenas, w.cfg.n_agents), dtype=torch.uint8, device="cuda")
        d_done = torch.zeros((arenas, w.cfg.n_agents), dtype=torch.uint8, device="cuda")
        cut = torch.zeros((), dtype=torch.int64, device="cuda")
        live = torch.zeros((), dtype=torch.int64, device="cuda")
        d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
        d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
        d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
        d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
        d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, device="cuda")
        d_probs = torch.empty((agents, 9), dtype=torch.float32, device="cuda")
        d_value = torch.empty(agents, dtype=torch.float32, device="cuda")
        d_cmd = torch.zeros(agents, dtype=torch.uint8, device="cuda")
        lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)

        def first_seeds(g):
            tb = (C.c_uint64 * arenas)(*[1_700_000_000 + g * arenas + a for a in range(arenas)])
            return tb, (C.c_uint64 * arenas)(*[123_456_789] * arenas)

        def play():
            sim.observe_sparse_device(*lists)
            sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
            net.predict_sparse(*lists, agents, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=1234,
                               d_dense_ptr=d_dense.data_ptr())
            sim.step_device(d_cmd.data_ptr(), 1)

        sim.reset(*first_seeds(0))
        net.reset_memory()
        stream.synchronize()
        t0 = time.perf_counter()
        if not whole_batch:
            next_game, d_tb_row = torch.zeros((1, arenas), dtype=torch.int64, device="cuda"), d_tb[None, :]
            for t in range(games * max_steps):
                if t % restart_every == 0:
                    sim.reset_arenas(done=True, max_steps=max_steps, tb_ptr=d_tb.data_ptr(), serial_ptr=d_serial.data_ptr(),
                                     selected_ptr=d_sel.data_ptr())
                    net.reset_memory(d_sel.data_ptr())
                    # three small tensor operations on the same stream: who is on which game, which seed comes next
                    game += d_sel[:, 0]
                    torch.remainder(game, games, out=next_game[0])
                    torch.gather(seed_list, 0, next_game, out=d_tb_row)
                if restart_every > 1:  # between two calls a finished arena stands still: count the arenas that play
                    sim.done_device(d_done.data_ptr())
                    live += (1 - d_done[:, 0].to(torch.int64)).sum()
                play()
            stream.synchronize()
            dt = time.perf_counter() - t0
            recs, (written, lost, pending) = sim.episodes()
            finished = written + lost + pending
            if restart_every == 1:
                live += games * max_steps * arenas  # every arena is in a running game whenever a step comes
            cut += int(game.sum().item()) - arenas - finished  # every restart followed a game that ended or one that was cut
        else:
            for g in range(games):
                if g:
                    sim.reset(*first_seeds(g))  # (synchronises; empties the log)
                    net.reset_memory()
                for _ in range(max_steps):
                    sim.done_device(d_done.data_ptr())
                    live += (1 - d_done[:, 0].to(torch.int64)).sum()  # a finished arena stands still until the round is over
                    play()
                sim.done_device(d_done.data_ptr())
                cut_host += int((1 - d_done[:, 0].to(torch.int64)).sum().item())  # still running when the round ends
                recs, (written, lost, pending) = sim.episodes()
                finished += written + lost + pending
            stream.synchronize()
            dt = time.perf_counter() - t0
        out = dict(arenas=arenas, games=games, max_steps=max_steps, ticks=games * max_steps, games_finished=int(finished),
                   games_cut=int(cut.item()) + cut_host, live_agent_steps=int(live.item()) * w.cfg.n_agents, seconds=dt)
        out["agent_steps_per_s"] = out["live_agent_steps"] / dt
    sim.set_stream(None), net.set_stream(None)
    net.close(), sim.close()
    return out


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    r = run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200,
            restart_every=int(sys.argv[4]) if len(sys.argv) > 4 else 1)
    print("%d arenas x %d ticks (%d seeds per arena, at most %d steps a game): %d games finished, %d cut by the limit, "
          "%.2f M agent-steps/s" % (r["arenas"], r["ticks"], r["games"], r["max_steps"], r["games_finished"], r["games_cut"],
                                    r["agent_steps_per_s"] / 1e6))
