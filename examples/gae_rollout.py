"""shaped_reward.py's loop with a rollout buffer that spans game ends, and GAE(lambda) over it: what a PPO learner is handed.

    python examples/gae_rollout.py [arenas] [steps] [T]

BASELINE configs[1] without auto_reset, the policy network, the shaped reward of `Signals.step` as the reward, and
`RolloutBatch(..., continuing=True)`: a restart never rewinds an agent, it is stored in `rb.first`, and all agents fill in
step, so every T-th tick is a hand-over and the host knows it without asking the device.  One tick, all on one stream:

    observe_sparse -> predict_sparse -> [every T-th tick: gae, ready_mask, release] -> step -> signals.step(reward)
                   -> record -> reset_arenas -> signals.step(rebase)

At a hand-over the block holds the T ticks before this one; this tick's value is the bootstrap value V_T and this tick's
restart flags say whether the game of slot T - 1 ended behind it (`gae(next_value=, next_mask=)`).  The record call stands
behind the step because the shaped reward of this tick's action exists only then.  There is no synchronisation in the loop.

The summary also says how many of the same run's ticks a per-game buffer of the same T (the reference Agent's rule: a restart
rewinds to slot 0, only a full buffer is handed over) would have handed to the learner: a game of L ticks fills
floor(L / T) buffers.  It is computed at the hand-overs from `rb.first` with a few torch operations, on the device.
The network's parameters are random here; the learner is the caller's.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy, rollout

arenas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
CAP, LIST_CAP, MAX_STEPS, GAMMA, LAMBDA = 2048, 512, 1000, 0.99, 0.95
SF_DIED, SF_WON = 1, 2
w = config.baseline_workload("C2", arenas=arenas, auto_reset=0)  # 64x64 map, 1 player + 16 zombies; restarts are ours
sim = env.ArenaBatch(w)
agents = arenas * w.cfg.n_agents
net = policy.PolicyBatch(policy.init_parameters(seed=0), agents)
rb = rollout.RolloutBatch(agents, T, LIST_CAP, continuing=True)
sig = sim.signals()
weights = env.reward_weights(per_step=-0.001, kills=1.0, damage=0.001, hp=0.002, died=-1.0, outcome={SF_DIED: -1.0, SF_WON: 5.0})
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
for x in (sim, net, rb):
    x.set_stream(stream.cuda_stream)
dev = dict(device="cuda")
d_keys = torch.zeros((agents, CAP), dtype=torch.int32, **dev)
d_vals = torch.zeros((agents, CAP), dtype=torch.float32, **dev)
d_counts = torch.zeros(agents, dtype=torch.int32, **dev)
d_pov = torch.zeros((agents, 160), dtype=torch.float32, **dev)
d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, **dev)
d_probs = torch.empty((agents, 9), dtype=torch.float32, **dev)
d_value = torch.empty(agents, dtype=torch.float32, **dev)
d_reward = torch.zeros(agents, dtype=torch.float32, **dev)
d_cmd = torch.zeros(agents, dtype=torch.uint8, **dev)
d_action = torch.zeros(agents, dtype=torch.int32, **dev)
d_ready = torch.zeros(agents, dtype=torch.uint8, **dev)
d_selected = torch.ones(agents, dtype=torch.uint8, **dev)  # every game is new at the first tick
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
out = tuple(torch.empty((T, agents), dtype=torch.float32, **dev) for _ in range(3))  # returns, V, advantages

# the per-game rule's yield, from the blocks' own flags
slot = torch.arange(T, **dev).unsqueeze(1)
game_len = torch.zeros(agents, dtype=torch.int64, **dev)  # ticks of each agent's running game in front of the block
per_game_buffers = torch.zeros((), dtype=torch.int64, **dev)
game_ends = torch.zeros((), dtype=torch.int64, **dev)
adv_sum = torch.zeros((), dtype=torch.float64, **dev)


def per_game_yield():
    """How many buffers of T the per-game rule fills inside this block: a game's ticks are numbered from its restart, and
    every T-th of them completes a buffer."""
    global game_len
    first = rb.first != 0
    last = torch.cummax(torch.where(first, slot, -1), dim=0).values  # the slot of the latest restart, -1: none in this block
    number = torch.where(last >= 0, slot - last, game_len + slot) + 1
    per_game_buffers.add_((number % T == 0).sum())
    game_ends.add_(first.sum())
    game_len = number[T - 1]


sim.reset(*w.seeds())
sig.step(rebase_ptr=d_selected)
handed = 0
sim.synchronize()
t0 = time.perf_counter()
for t in range(steps):
    sim.observe_sparse_device(*lists)
    sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
    net.predict_sparse(*lists, agents, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr(),
                       d_dense_ptr=d_dense.data_ptr(), d_reset_mask_ptr=d_selected.data_ptr())
    if t and t % T == 0:  # the hand-over: every agent's buffer is full, this tick is the one behind slot T - 1
        rb.gae(GAMMA, LAMBDA, next_value=d_value, next_mask=d_selected, out=out)
        rb.ready_mask(d_ready)
        # ... a learner's epochs over rb.state(t), rb.action, rb.logp, rb.first, the returns and the advantages go here
        # (examples/dense_epoch.py: the states as dense rows for a torch module, rb.dense(t)) ...
        adv_sum += out[2].sum(dtype=torch.float64)
        per_game_yield()
        rb.release()
        handed += 1
    sim.step_device(d_cmd.data_ptr(), 1)
    sig.step(reward_ptr=d_reward, weights=weights)                  # what this tick's action earned
    rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_action.data_ptr(), d_reward.data_ptr(), *lists, d_reset_mask_ptr=d_selected.data_ptr())
    sim.reset_arenas(done=True, max_steps=MAX_STEPS, selected_ptr=d_selected.data_ptr())
    sig.step(rebase_ptr=d_selected)
sim.synchronize(), net.synchronize(), rb.synchronize()
dt = time.perf_counter() - t0
ready, dropped, missing = rb.status()
stored = handed * T * agents
assert dropped == 0 and int(d_ready.sum().item()) == (agents if handed else 0)
print("%d arenas x %d steps, T = %d, gamma %.2f lambda %.2f: %.2f M agent-steps/s; %d hand-overs of %d agents = %d ticks handed to the "
      "learner, %d game ends inside them, mean advantage %.5f; a per-game buffer of the same T would have handed over %d of those "
      "ticks (%.1f %%); %d states whose list did not fit %d entries"
      % (arenas, steps, T, GAMMA, LAMBDA, agents * steps / dt / 1e6, handed, agents, stored, int(game_ends.item()),
         float(adv_sum.item()) / max(stored, 1), int(per_game_buffers.item()) * T, 100.0 * int(per_game_buffers.item()) * T / max(stored, 1),
         missing, LIST_CAP))
sig.close()
