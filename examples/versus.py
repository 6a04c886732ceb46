"""Two parameter sets in one match, nothing leaving HBM: observe -> gather -> one network per side -> scatter -> step.

    python examples/versus.py [arenas] [steps]

The `KITS` Battle workload (6 commanded humans per arena, teams 1,2,3,1,2,3).  Every commanded human of the reference owns
its network (bots/bot-0.5/Custom.hpp:161-165, bots/bot-1/Agent.hpp:84-101); here `policy.Router` assigns the agents of the
whole batch to two `PolicyBatch` objects by team parity (teams 1 and 3: network 1, team 2: network 0), each network
evaluates only its own agents, and each has a seed of its own: behind a route the draw of slot s is keyed by (seed, s, i).
The episode log is on; a finished game counts for the network whose agents hold more Hp in sum at its end than the other's
(a tie, or nobody alive: for neither).  The parameters are random here: pass two checkpoints (policy.load_checkpoint) to
compare learners.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy

arenas = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
w = config.baseline_workload("KITS", arenas=arenas)
n = w.cfg.n_agents
agents = arenas * n
teams = [1, 2, 3, 1, 2, 3]
assign = [teams[a % n] % 2 for a in range(agents)]
CAP = 2048
sim = env.ArenaBatch(w)
router = policy.Router(assign, 2, cap=CAP, dense=True)
nets = [policy.PolicyBatch(policy.init_parameters(seed=k), router.count(k)) for k in range(2)]
seeds = [1234, 98765]
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
for x in [sim, router] + nets:
    x.set_stream(stream.cuda_stream)
sim.enable_episode_log(64)
sim.reset(*w.seeds())
d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, device="cuda")  # rows only for lists that do not fit
d_cmd = torch.zeros(agents, dtype=torch.uint8, device="cuda")
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
restarted = sim.done_view_device()
records = []
t0 = time.perf_counter()
for t in range(steps):
    sim.observe_sparse_device(*lists)
    sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
    router.gather(lists, d_dense_ptr=d_dense.data_ptr(), reset_words=restarted)   # every network's agents into its own rows
    for k in range(2):                                                              # Agent::predict + update, per network
        nets[k].predict_sparse(**router.inputs(k), **router.outputs(k), seed=seeds[k])
    router.scatter({"cmd": d_cmd})                                                  # the commands back in the environment's order
    sim.step_device(d_cmd.data_ptr(), 1)
    if t % 50 == 49:  # (a ring of 64 per arena: fetched long before it can wrap)
        records.append(sim.episodes()[0])
sim.synchronize()
dt = time.perf_counter() - t0
records.append(sim.episodes()[0])
ep = env.decode_episodes(np.concatenate(records), n)
games = len(ep["arena"])
hp = np.maximum(ep["results"][:, :, 5], 0) if games else np.zeros((0, n), dtype=np.int64)
side = np.array(assign[:n])
hp0, hp1 = hp[:, side == 0].sum(axis=1), hp[:, side == 1].sum(axis=1)
won = [int((hp0 > hp1).sum()), int((hp1 > hp0).sum())]
share = [x / games if games else 0.0 for x in won]
print("%d arenas x %d steps in %.2f s = %.2f M agent-steps/s; %d games finished: network 0 (%d agents per arena) won %.3f, "
      "network 1 (%d agents per arena) won %.3f, neither %.3f"
      % (arenas, steps, dt, agents * steps / dt / 1e6, games, int((side == 0).sum()), share[0], int((side == 1).sum()), share[1],
         1.0 - share[0] - share[1] if games else 0.0))
