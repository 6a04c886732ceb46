"""ppo_rollout.py's loop with a reward shaped from the game's own counters in place of bot-1's `log D`.

    python examples/shaped_reward.py [arenas] [steps] [T] [max_steps]

One tick, all on one stream and with nothing leaving HBM:

    observe_sparse -> predict_sparse -> step -> signals.step(reward) -> rollout.record -> reset_arenas -> signals.step(rebase)

`Signals.step` behind the step turns what the tick changed — kills, team kills, loot, damage dealt, effect, Hp lost, a
death, the game's outcome (strikeforce.h sf_signals_step) — into one float per agent in the layout `RolloutBatch.record`
takes as its reward.  The games run without auto_reset: `reset_arenas(done=True, max_steps=...)` restarts the finished
games, and cuts the ones that ran too long, on the device, and writes which agents it restarted to a mask
(selected_ptr=).  That mask is what the policy's memory reset and the rollout buffer take as restart flags at the next
tick, and it goes to the signals object as d_rebase in a second call without outputs, right behind the restart: the
restarted agents' baselines become the new games' first states (rule 1), so that neither the cut game's counters nor the
new game's first tick are lost or mixed.  The finished games' last deltas and outcomes were handed out by the first call,
before the restart.  The network's parameters are random here; the learner is the caller's.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy, rollout

arenas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
max_steps = int(sys.argv[4]) if len(sys.argv) > 4 else 150
CAP, LIST_CAP, CHECK_EVERY = 2048, 512, 16
SF_DIED, SF_WON = 1, 2
w = config.baseline_workload("C2", arenas=arenas, auto_reset=0)  # 64x64 map, 1 player + 16 zombies; restarts are ours
sim = env.ArenaBatch(w)
agents = arenas * w.cfg.n_agents
net = policy.PolicyBatch(policy.init_parameters(seed=0), agents)
rb = rollout.RolloutBatch(agents, T, LIST_CAP)
sig = sim.signals()
# +1 per kill, a little for damage dealt, a little less for every Hp lost, -1 for dying, +5 for winning, -0.001 per tick
weights = env.reward_weights(per_step=-0.001, kills=1.0, damage=0.001, hp=0.002, died=-1.0, outcome={SF_DIED: -1.0, SF_WON: 5.0})
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
for x in (sim, net, rb):
    x.set_stream(stream.cuda_stream)
d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, device="cuda")
d_probs = torch.empty((agents, 9), dtype=torch.float32, device="cuda")
d_value = torch.empty(agents, dtype=torch.float32, device="cuda")
d_reward = torch.zeros(agents, dtype=torch.float32, device="cuda")
d_delta = torch.zeros((arenas, w.cfg.n_agents, 8), dtype=torch.int32, device="cuda")
d_cmd = torch.zeros(agents, dtype=torch.uint8, device="cuda")
d_action = torch.zeros(agents, dtype=torch.int32, device="cuda")
d_ready = torch.zeros(agents, dtype=torch.uint8, device="cuda")
d_selected = torch.ones(agents, dtype=torch.uint8, device="cuda")  # every game is new at the first tick
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)

sim.reset(*w.seeds())
sig.step(rebase_ptr=d_selected)                                  # the baselines of the first games
reward_sum = torch.zeros((), dtype=torch.float64, device="cuda")
ended = torch.zeros((), dtype=torch.int64, device="cuda")
out, trained = None, 0
sim.synchronize()
t0 = time.perf_counter()
for t in range(steps):
    sim.observe_sparse_device(*lists)
    sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
    net.predict_sparse(*lists, agents, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr(),
                       d_dense_ptr=d_dense.data_ptr(), d_reset_mask_ptr=d_selected.data_ptr())
    sim.step_device(d_cmd.data_ptr(), 1)
    sig.step(delta_ptr=d_delta, reward_ptr=d_reward, weights=weights)   # what this tick's action earned
    rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_action.data_ptr(), d_reward.data_ptr(), *lists,
              d_reset_mask_ptr=d_selected.data_ptr())
    reward_sum += d_reward.sum(dtype=torch.float64)
    ended += ((d_delta[:, :, 0] & env.SIG_ENDED) != 0).sum()
    # finished games, and games of max_steps ticks, start again on the next seed; the agents restarted go to d_selected
    sim.reset_arenas(done=True, max_steps=max_steps, selected_ptr=d_selected.data_ptr())
    sig.step(rebase_ptr=d_selected)                              # no outputs: only the restarted agents' baselines move
    if t % CHECK_EVERY == CHECK_EVERY - 1 and rb.status()[0]:
        out = rb.returns(0.99, out=out)
        rb.ready_mask(d_ready)
        # ... a learner's epochs over the ready agents' columns go here ...
        net.reset_memory(d_ready.data_ptr())
        trained += int(d_ready.sum().item())
        rb.release()
sim.synchronize(), net.synchronize(), rb.synchronize()
dt = time.perf_counter() - t0
unresolved, detected = sig.status()
print("%d arenas x %d steps, T = %d: %.2f M agent-steps/s; %d games ended, mean shaped reward per tick %.5f; %d buffers handed "
      "over; signals: %d unresolved, %d rebased by detection (every restart was announced)"
      % (arenas, steps, T, agents * steps / dt / 1e6, int(ended.item()), float(reward_sum.item()) / (agents * steps), trained,
         unresolved, detected))
sig.close()
