"""k_tail of a reward object against k_tail of a policy object, one process, the same lists:

    python tools/reward_tail_time.py [out.json]

For 4096 and 16 384 agents of BASELINE configs[1] 100 steps in: the list-form forward of a PolicyBatch and of a RewardBatch
(same parameters, same lists, the actions of one predict call), 21 repeats each, interleaved policy / reward / policy, so that
the second policy series gives the spread between repeats of one figure.  Times are the library's own device events around
the launch (sf_policy_kernel_time_by_kernel, index 3 = k_tail, index 2 = k_feat_list).  Prints one JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy

REPS, CAP = 21, 2048
out = {"reps": REPS, "unit": "ms per launch, device events", "sizes": {}}
params = policy.init_parameters(seed=0)
for agents in (4096, 16384):
    w = config.baseline_workload("C2", arenas=agents)
    sim = env.ArenaBatch(w)
    assert w.cfg.n_agents == 1
    sim.reset(*w.seeds())
    cmds, _ = config.bench_commands(agents, 1, 100)
    d_cmds = torch.from_numpy(np.ascontiguousarray(cmds)).cuda()
    sim.step_device(d_cmds.data_ptr(), 100)
    i32 = dict(dtype=torch.int32, device="cuda")
    d_keys, d_counts, d_act = torch.zeros((agents, CAP), **i32), torch.zeros(agents, **i32), torch.zeros(agents, **i32)
    d_vals, d_pov = torch.zeros((agents, CAP), device="cuda"), torch.zeros((agents, 160), device="cuda")
    d_probs, d_value = torch.zeros((agents, 9), device="cuda"), torch.zeros(agents, device="cuda")
    d_disc, d_rew, d_cmd = torch.zeros(agents, device="cuda"), torch.zeros(agents, device="cuda"), torch.zeros(agents, dtype=torch.uint8, device="cuda")
    sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
    sim.synchronize()
    assert int(d_counts.max().item()) <= CAP
    net, rew = policy.PolicyBatch(params, agents), policy.RewardBatch(params, agents)
    la = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr())
    net.predict_sparse(*la, CAP, agents, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=3, d_action_ptr=d_act.data_ptr())
    net.synchronize()

    def policy_once():
        net.forward_sparse(*la, CAP, agents, d_probs.data_ptr(), d_value.data_ptr())

    def reward_once():
        rew.reward_sparse(*la, CAP, agents, d_act.data_ptr(), d_disc.data_ptr(), d_rew.data_ptr())

    def timed(obj, once):
        obj.kernel_time_by_kernel(True)
        once()
        k = obj.kernel_time_by_kernel(False)
        assert k[3][2] == 1 and k[2][2] == 1
        return k[3][0], k[2][0]

    for _ in range(5):
        policy_once(), reward_once()
    net.synchronize(), rew.synchronize()
    series = {"policy": [], "reward": [], "policy_again": []}
    for _ in range(REPS):
        series["policy"].append(timed(net, policy_once))
        series["reward"].append(timed(rew, reward_once))
        series["policy_again"].append(timed(net, policy_once))
    row = {"mean_list_entries": float(d_counts.float().mean().item())}
    for name, v in series.items():
        tail, feat = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        row[name] = {"k_tail_median": float(np.median(tail)), "k_tail_min": float(tail.min()), "k_tail_max": float(tail.max()),
                     "k_feat_list_median": float(np.median(feat))}
    row["reward_over_policy"] = row["reward"]["k_tail_median"] / row["policy"]["k_tail_median"]
    row["policy_again_over_policy"] = row["policy_again"]["k_tail_median"] / row["policy"]["k_tail_median"]
    out["sizes"][str(agents)] = row
    net.close(), rew.close(), sim.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
