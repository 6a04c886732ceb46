"""gae_rollout.py's loop with the pass a learner's epoch makes over the stored states: `rb.dense(t)` feeds a torch module.

    python examples/dense_epoch.py [arenas] [steps] [T] [bf16]

BASELINE configs[1] without auto_reset, the policy network, the shaped reward, `RolloutBatch(..., continuing=True)`, GAE at
every hand-over — as in gae_rollout.py, at a small T.  At each hand-over the block's states are walked the way the
reference's epochs walk them (`model->forward(states[i])` for i = 0..T-1, bots/bot-1/Agent.hpp:392, RewardNet.hpp:265-274):
for every slot t, `rb.dense(t)` expands the stored lists into dense `[rows, 32, 31, 31]` rows, at most CHUNK rows per call
(a call takes up to rollout.DENSE_ROWS_MAX; a chunk bounds the memory of the dense batch), and a torch module consumes
them.  The module stands where a learner's model would: four bias-free stride-2 conv2d with random weights, no gradients of
the library's, no optimiser.  Rows whose list did not fit (`valid == 0`) come out all zero; the example counts them.
With `bf16` the rows are written as bfloat16 in torch's channels_last format and the module runs in that type.
Prints the rows per second of the epoch pass (expansion and module, device events around each hand-over's pass).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy, rollout

arenas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(sys.argv[3]) if len(sys.argv) > 3 else 16
half = len(sys.argv) > 4 and sys.argv[4] == "bf16"
CAP, LIST_CAP, MAX_STEPS, GAMMA, LAMBDA, CHUNK = 2048, 512, 1000, 0.99, 0.95, 4096
SF_DIED, SF_WON = 1, 2
w = config.baseline_workload("C2", arenas=arenas, auto_reset=0)
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
d_selected = torch.ones(agents, dtype=torch.uint8, **dev)
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
out = tuple(torch.empty((T, agents), dtype=torch.float32, **dev) for _ in range(3))  # returns, V, advantages

# the stand-in for a learner's model, and the dense batch it reads (allocated once, written by every rb.dense call)
dtype = torch.bfloat16 if half else torch.float32
torch.manual_seed(0)
model = torch.nn.Sequential(*[torch.nn.Conv2d(c, 2 * c, 3, stride=2, bias=False) for c in (32, 64, 128, 256)]).to("cuda", dtype)
chunk = min(CHUNK, agents, rollout.DENSE_ROWS_MAX)
batch = torch.empty((chunk, 31, 31, 32) if half else (chunk, 32, 31, 31), dtype=dtype, **dev)
valid = torch.empty(chunk, dtype=torch.uint8, **dev)
if half:
    model = model.to(memory_format=torch.channels_last)
seen = torch.zeros((), dtype=torch.float64, **dev)
blank = torch.zeros((), dtype=torch.int64, **dev)
spans, rows_done = [], 0


def epoch_pass():
    """One walk over the block: every slot, every agent, in chunks."""
    global rows_done
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    with torch.no_grad():
        for t in range(T):
            for agent0 in range(0, agents, chunk):
                rows = min(chunk, agents - agent0)
                x, ok = rb.dense(t, agent0=agent0, rows=rows, dtype=dtype, channels_last=half, out=batch, valid=valid)
                y = model(x[:rows])  # ... a learner's forward, loss and backward on slot t's rows go here ...
                seen.add_(y.float().abs().sum(dtype=torch.float64))
                blank.add_(rows - ok[:rows].sum())
                rows_done += rows
    b.record()
    spans.append((a, b))


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
    if t and t % T == 0:  # the hand-over: every agent's buffer is full
        rb.gae(GAMMA, LAMBDA, next_value=d_value, next_mask=d_selected, out=out)
        epoch_pass()
        rb.release()
        handed += 1
    sim.step_device(d_cmd.data_ptr(), 1)
    sig.step(reward_ptr=d_reward, weights=weights)
    rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_action.data_ptr(), d_reward.data_ptr(), *lists, d_reset_mask_ptr=d_selected.data_ptr())
    sim.reset_arenas(done=True, max_steps=MAX_STEPS, selected_ptr=d_selected.data_ptr())
    sig.step(rebase_ptr=d_selected)
sim.synchronize(), net.synchronize(), rb.synchronize()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
ms = sum(a.elapsed_time(b) for a, b in spans)
ready, dropped, missing = rb.status()
assert dropped == 0 and rows_done == handed * T * agents
print("%d arenas x %d steps, T = %d, %s: %d hand-overs; the epoch pass expanded %d rows in chunks of %d and ran the module on them in "
      "%.1f ms: %.0f rows/s (%d rows all zero because their list did not fit %d entries; sum |module output| %.6g); whole loop %.2f s"
      % (arenas, steps, T, "bfloat16 channels_last" if half else "float32 NCHW", handed, rows_done, chunk, ms,
         rows_done / max(ms, 1e-9) * 1e3, int(blank.item()), LIST_CAP, float(seen.item()), dt))
sig.close()
