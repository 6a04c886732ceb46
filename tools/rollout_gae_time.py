"""What sf_rollout_gae and the continuing record launch cost against the calls they stand beside ("The rollout
buffer across game ends"), one process:

    python tools/rollout_gae_time.py [out.json]

1. sf_rollout_gae in the reference configuration (lambda = 1, log_values, reward_scale = 1.f - gamma, no next value, `first`
   all zero; returns, V and advantages written) against sf_rollout_returns (returns, log V and advantages written, no
   statistics) on the same buffer: 4096 agents, T = 1024, all ready.  Two series of each, the four calls alternating and the
   order rotating by one every repeat; device events around each call; medians of 21 after 10 warm-up rounds.
2. The continuing record launch against the per-game one in the closed loop of BASELINE configs[1]: 4096 agents, T = 1024,
   list_cap = 512, two rollouts fed by the same tick; per tick each is recorded twice (series a and b), the four launches
   alternating and rotating as above; device events around each launch.
The two series of a yardstick (sf_rollout_returns, the per-game record) give its spread: |median a - median b|.  The new
call passes when its median is no larger than the yardstick's (series a against series a) plus that spread.
Prints one JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy, rollout

REPS, WARM, CAP, AGENTS, T, LIST_CAP, GAMMA = 21, 10, 2048, 4096, 1024, 512, 0.99
out = {"reps": REPS, "warm": WARM, "unit": "ms, device events", "agents": AGENTS, "T": T}


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


def alternate(calls, before=None):
    """calls: name -> function.  WARM rounds untimed, then REPS rounds with every call timed, the order rotating."""
    names = list(calls)
    spans = {n: [] for n in names}
    for i in range(WARM + REPS):
        if before:
            before()
        for k in range(len(names)):
            n = names[(i + k) % len(names)]
            if i < WARM:
                calls[n]()
            else:
                spans[n].append(span(calls[n]))
    return {n: med(v) for n, v in spans.items()}


def verdict(row, new, yard):
    spread = abs(row[yard + "_a"]["median"] - row[yard + "_b"]["median"])
    row["yardstick_spread_ms"] = spread
    row["new_over_yardstick"] = row[new + "_a"]["median"] / row[yard + "_a"]["median"]
    row["within_bound"] = bool(row[new + "_a"]["median"] <= row[yard + "_a"]["median"] + spread)


# ---- 1. sf_rollout_gae against sf_rollout_returns -----------------------------------------------------------------------
rb = rollout.RolloutBatch(AGENTS, T, 8, store_states=False, continuing=True)
rng = np.random.default_rng(0)
rewards = torch.from_numpy(np.log(rng.uniform(1e-3, 1, size=(T, AGENTS))).astype(np.float32)).cuda()
values = torch.from_numpy(rng.uniform(1e-3, 1, size=(T, AGENTS)).astype(np.float32)).cuda()
actions = torch.from_numpy(rng.integers(0, 9, size=(T, AGENTS)).astype(np.int32)).cuda()
probs = torch.full((AGENTS, 9), 1 / 9, device="cuda")
for t in range(T):
    rb.record(probs.data_ptr(), values[t].data_ptr(), actions[t].data_ptr(), rewards[t].data_ptr())
assert rb.status()[0] == AGENTS and int(rb.first.sum().item()) == 0
scale = float(np.float32(1) - np.float32(GAMMA))
new = lambda: tuple(torch.empty((T, AGENTS), device="cuda") for _ in range(3))
res_r, res_g = new() + (None,), new()
returns = lambda: rb.returns(GAMMA, out=res_r)
gae = lambda: rb.gae(GAMMA, 1.0, reward_scale=scale, log_values=True, out=res_g)
row = alternate({"returns_a": returns, "gae_a": gae, "returns_b": returns, "gae_b": gae})
rb.synchronize()
row["same_bits"] = bool(all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res_r[:3], res_g)))
# bytes: reward and value read, three arrays written; gae also writes V and reads it again, and reads `first`
row["bytes_returns"], row["bytes_gae"] = T * AGENTS * 20, T * AGENTS * 25
verdict(row, "gae", "returns")
out["gae_vs_returns"] = row
rb.close()
del rb, res_r, res_g

# ---- 2. the continuing record launch against the per-game one -----------------------------------------------------------
w = config.baseline_workload("C2", arenas=AGENTS)
assert w.cfg.n_agents == 1
sim = env.ArenaBatch(w)
sim.reset(*w.seeds())
net, disc = policy.PolicyBatch(policy.init_parameters(seed=0), AGENTS), policy.RewardBatch(policy.init_parameters(seed=1), AGENTS)
rb_game, rb_cont = rollout.RolloutBatch(AGENTS, T, LIST_CAP), rollout.RolloutBatch(AGENTS, T, LIST_CAP, continuing=True)
i32 = dict(dtype=torch.int32, device="cuda")
d_keys, d_counts, d_act = torch.zeros((AGENTS, CAP), **i32), torch.zeros(AGENTS, **i32), torch.zeros(AGENTS, **i32)
d_vals, d_pov = torch.zeros((AGENTS, CAP), device="cuda"), torch.zeros((AGENTS, 160), device="cuda")
d_probs, d_value, d_rew = torch.zeros((AGENTS, 9), device="cuda"), torch.zeros(AGENTS, device="cuda"), torch.zeros(AGENTS, device="cuda")
d_cmd = torch.zeros(AGENTS, dtype=torch.uint8, device="cuda")
restarted = sim.done_view_device()
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)


def tick():
    sim.step_device(d_cmd.data_ptr(), 1)
    sim.observe_sparse_device(*lists)
    net.predict_sparse(*lists, AGENTS, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=7, d_action_ptr=d_act.data_ptr(),
                       reset_words=restarted)
    disc.reward_sparse(*lists, AGENTS, d_act.data_ptr(), d_reward_ptr=d_rew.data_ptr(), reset_words=restarted)


rec = lambda rb: (lambda: rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists, reset_words=restarted))
row = alternate({"per_game_a": rec(rb_game), "continuing_a": rec(rb_cont), "per_game_b": rec(rb_game), "continuing_b": rec(rb_cont)}, before=tick)
for rb in (rb_game, rb_cont):
    ready, dropped, missing = rb.status()
    assert ready == 0 and dropped == 0, (ready, dropped)
assert int(rb_cont.fill().min().item()) == 2 * (WARM + REPS)
row.update(list_cap=LIST_CAP, mean_list_entries=float(d_counts.float().mean().item()), missing_states=missing)
verdict(row, "continuing", "per_game")
out["record_continuing_vs_per_game"] = row
for x in (rb_game, rb_cont, net, disc, sim):
    x.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
