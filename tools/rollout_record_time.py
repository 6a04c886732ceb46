"""What the rollout buffer costs ("The rollout buffer"), one process:

    python tools/rollout_record_time.py [out.json]

1. sf_rollout_record per tick in the closed loop of examples/ppo_rollout.py: 4096 agents of BASELINE configs[1], T = 256,
   list_cap = 512.  Ticks alternate without / with / without the record call; device events around every tick, and around
   the record launch alone; medians of 21 after 10 warm-up ticks.  The second without-series gives the spread between
   repeats of one figure.  Bytes the launch must move (read + write) are counted from the tick's own list counts.
2. sf_rollout_returns at T = 1024, 4096 agents, every agent ready: device events around the launch, median of 21.
Prints one JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy, rollout

REPS, WARM, CAP, AGENTS = 21, 10, 2048, 4096
HBM_TBS = 6.3  # what a float4 copy reaches on this part: the rate the byte counts are set against
out = {"reps": REPS, "unit": "ms, device events", "hbm_rate_TB_s": HBM_TBS}


def span(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def med(pairs):
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in pairs])
    return {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


# ---- 1. record in the closed loop ---------------------------------------------------------------------------------------
T, LIST_CAP = 256, 512
w = config.baseline_workload("C2", arenas=AGENTS)
assert w.cfg.n_agents == 1
sim = env.ArenaBatch(w)
sim.reset(*w.seeds())
net, disc = policy.PolicyBatch(policy.init_parameters(seed=0), AGENTS), policy.RewardBatch(policy.init_parameters(seed=1), AGENTS)
rb = rollout.RolloutBatch(AGENTS, T, LIST_CAP)
i32 = dict(dtype=torch.int32, device="cuda")
d_keys, d_counts, d_act = torch.zeros((AGENTS, CAP), **i32), torch.zeros(AGENTS, **i32), torch.zeros(AGENTS, **i32)
d_vals, d_pov = torch.zeros((AGENTS, CAP), device="cuda"), torch.zeros((AGENTS, 160), device="cuda")
d_probs, d_value, d_rew = torch.zeros((AGENTS, 9), device="cuda"), torch.zeros(AGENTS, device="cuda"), torch.zeros(AGENTS, device="cuda")
d_cmd = torch.zeros(AGENTS, dtype=torch.uint8, device="cuda")
restarted = sim.done_view_device()
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
record_spans, record_bytes = [], []


def tick(with_record, timed=False):
    sim.observe_sparse_device(*lists)
    net.predict_sparse(*lists, AGENTS, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=7, d_action_ptr=d_act.data_ptr(),
                       reset_words=restarted)
    disc.reward_sparse(*lists, AGENTS, d_act.data_ptr(), d_reward_ptr=d_rew.data_ptr(), reset_words=restarted)
    if with_record:
        call = lambda: rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists, reset_words=restarted)
        if timed:
            record_spans.append(span(call))
            record_bytes.append(torch.clamp(d_counts, max=LIST_CAP).to(torch.int64).sum())  # (read on the host after the series)
        else:
            call()
    sim.step_device(d_cmd.data_ptr(), 1)


for i in range(WARM):
    tick(i % 2 == 1)
series = {"without": [], "with": [], "without_again": []}
for _ in range(REPS):
    series["without"].append(span(lambda: tick(False)))
    series["with"].append(span(lambda: tick(True, timed=True)))
    series["without_again"].append(span(lambda: tick(False)))
row = {k: med(v) for k, v in series.items()}
row["record_launch"] = med(record_spans)
ready, dropped, missing = rb.status()
assert ready == 0 and dropped == 0, (ready, dropped)
# per agent: the list entries (8 B each) and pov (640 B) read and written; probs 36 + logp 36; action, value, reward and
# count twice; the cursor twice; the restart word
b = float(np.median([int(n.item()) * 16 + AGENTS * (2 * 640 + 72 + 4 * 8 + 8 + 4) for n in record_bytes]))
row.update(T=T, list_cap=LIST_CAP, agents=AGENTS, mean_list_entries=float(d_counts.float().mean().item()), missing_states=missing,
           bytes_per_tick=b, bytes_over_hbm_rate_ms=b / (HBM_TBS * 1e12) * 1e3,
           with_minus_without_ms=row["with"]["median"] - row["without"]["median"],
           without_again_over_without=row["without_again"]["median"] / row["without"]["median"])
out["record"] = row
for x in (rb, net, disc, sim):
    x.close()
del rb

# ---- 2. returns at T = 1024 ---------------------------------------------------------------------------------------------
T = 1024
rb = rollout.RolloutBatch(AGENTS, T, 8, store_states=False)
rng = np.random.default_rng(0)
rewards = torch.from_numpy(np.log(rng.uniform(1e-3, 1, size=(T, AGENTS))).astype(np.float32)).cuda()
values = torch.from_numpy(rng.uniform(1e-3, 1, size=(T, AGENTS)).astype(np.float32)).cuda()
actions = torch.from_numpy(rng.integers(0, 9, size=(T, AGENTS)).astype(np.int32)).cuda()
probs = torch.full((AGENTS, 9), 1 / 9, device="cuda")
for t in range(T):
    rb.record(probs.data_ptr(), values[t].data_ptr(), actions[t].data_ptr(), rewards[t].data_ptr())
assert rb.status()[0] == AGENTS
res = rb.returns(0.99)
for _ in range(3):
    rb.returns(0.99, out=res)
spans = [span(lambda: rb.returns(0.99, out=res)) for _ in range(REPS)]
row = med(spans)
b = T * AGENTS * 24 + AGENTS * 20  # reward, value, action read once; returns, log V, advantage written; cursor + four statistics
row.update(T=T, agents=AGENTS, bytes=b, bytes_over_hbm_rate_ms=b / (HBM_TBS * 1e12) * 1e3)
out["returns"] = row
rb.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
