"""The closed loop of examples/policy_loop.py with invalid-action masking, nothing leaving HBM:
observe -> bot-0.5 network -> action mask -> masked draw -> step.

    python examples/masked_policy_loop.py [arenas] [steps]

sf_action_mask_device says which of the bot's nine commands obey() would not silently drop right now (a step into a wall, a
shot with the bullet pool dry, ...), and sf_policy_act_masked draws among those only.  The fused predict_sparse draws unmasked,
so the masked loop is reset_memory + forward_sparse + action_mask + act_masked: two launches more per tick.  At the end the
share of drawn commands that were effective — whose bit was set in the mask of the state they were drawn for — is printed for
a run with the mask and a run without it (same network, same seeds).  The mask is of the stored state: zombies, bullets and
the humans earlier in the sweep still move before a command is obeyed, so "effective" is what obey would do now, not a promise.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy

arenas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
CAP = 2048


def run(masked):
    w = config.baseline_workload("C2", arenas=arenas)       # 64x64 map, 1 player + 16 zombies, auto-reset
    sim = env.ArenaBatch(w)
    agents = arenas * w.cfg.n_agents
    net = policy.PolicyBatch(policy.init_parameters(seed=0), agents)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sim.set_stream(stream.cuda_stream), net.set_stream(stream.cuda_stream)
    sim.reset(*w.seeds())
    d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
    d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
    d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
    d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, device="cuda")
    d_probs = torch.empty((agents, 9), dtype=torch.float32, device="cuda")
    d_value = torch.empty(agents, dtype=torch.float32, device="cuda")
    d_cmd = torch.zeros(agents, dtype=torch.uint8, device="cuda")
    d_action = torch.zeros(agents, dtype=torch.int32, device="cuda")
    d_done = torch.zeros(agents, dtype=torch.uint8, device="cuda")
    effective = torch.zeros((), dtype=torch.int64, device="cuda")
    t0 = time.perf_counter()
    for t in range(steps):
        sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
        sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
        sim.done_device(d_done.data_ptr())                   # a new Agent's memory for the games that just restarted
        net.reset_memory(d_done.data_ptr(), agents)
        net.forward_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, agents,
                           d_probs.data_ptr(), d_value.data_ptr(), d_dense_ptr=d_dense.data_ptr())
        _, actions = sim.action_mask(policy.ACTION_STRING)   # bit j: ACTION_STRING[j] would do something
        if masked:
            net.act_masked(d_probs.data_ptr(), agents, actions.data_ptr(), d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr())
        else:
            net.act(d_probs.data_ptr(), agents, d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr())
        effective += ((actions.reshape(-1) >> d_action) & 1).sum()   # (bookkeeping of this example, on the same stream)
        sim.step_device(d_cmd.data_ptr(), 1)
    sim.synchronize(), net.synchronize()
    dt = time.perf_counter() - t0
    share = float(effective.item()) / (agents * steps)
    kills = int(sim.results()[:, :, 0].sum())
    sim.close()
    return share, agents * steps / dt / 1e6, kills


for masked in (True, False):
    share, rate, kills = run(masked)
    print("%s the mask: %5.1f %% of %d drawn commands were effective; %.2f M agent-steps/s; kills so far: %d"
          % ("with   " if masked else "without", 100 * share, arenas * steps, rate, kills))
