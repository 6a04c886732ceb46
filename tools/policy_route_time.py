"""What routing agents to two networks costs ("Several networks in one match"), one process:

    python tools/policy_route_time.py [out.json]

BASELINE configs[4] (8 commanded humans per arena) at 4096 arenas, two networks of 4 seats each (even seats: network 0).
Three closed-loop ticks, each observe -> networks -> step on one stream, device events around whole ticks, medians of 21
after 10 warm-up ticks, the three forms alternating so that they see the same games:
  routed         gather, one predict_sparse per network on its 16 384 agents, scatter of the commands
  everybody      both networks evaluate all 32 768 agents (the parent commit's entries only); the commands are selected per
                 agent on the device (torch.where)
  one_network    one network evaluates all 32 768 agents, no routing
and device events around the gather and the scatter launch alone, with the bytes each must move (read + write, from the
tick's own list counts) and those bytes at 6.3 TB/s.  Prints one JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy

REPS, WARM, CAP, ARENAS = 21, 10, 2048, 4096
HBM_TBS = 6.3  # what a float4 copy reaches on this part: the rate the byte counts are set against
w = config.baseline_workload("C5", arenas=ARENAS)
N = w.cfg.n_agents
AGENTS = ARENAS * N
assert N == 8
assign = [a % 2 for a in range(AGENTS)]
sim = env.ArenaBatch(w)
router = policy.Router(assign, 2, cap=CAP)
half = [policy.PolicyBatch(policy.init_parameters(seed=k), router.count(k)) for k in range(2)]
full = [policy.PolicyBatch(policy.init_parameters(seed=k), AGENTS) for k in range(2)]
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
for x in [sim, router] + half + full:
    x.set_stream(stream.cuda_stream)
sim.reset(*w.seeds())
i32 = dict(dtype=torch.int32, device="cuda")
d_keys, d_counts = torch.zeros((AGENTS, CAP), **i32), torch.zeros(AGENTS, **i32)
d_vals, d_pov = torch.zeros((AGENTS, CAP), device="cuda"), torch.zeros((AGENTS, 160), device="cuda")
d_probs = [torch.zeros((AGENTS, 9), device="cuda") for _ in range(2)]
d_value = [torch.zeros(AGENTS, device="cuda") for _ in range(2)]
d_cmds = [torch.zeros(AGENTS, dtype=torch.uint8, device="cuda") for _ in range(2)]
d_cmd = torch.zeros(AGENTS, dtype=torch.uint8, device="cuda")
d_owner = torch.tensor(assign, dtype=torch.uint8, device="cuda") == 0
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
restarted = sim.done_view_device()
gather_spans, scatter_spans, gather_entries = [], [], []


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


def routed(timed=False):
    sim.observe_sparse_device(*lists)
    call = lambda: router.gather(lists, reset_words=restarted)
    if timed:
        gather_spans.append(span(call))
    else:
        call()
    for k in range(2):
        half[k].predict_sparse(**router.inputs(k), **router.outputs(k), seed=100 + k)
    call = lambda: router.scatter({"cmd": d_cmd})
    if timed:
        scatter_spans.append(span(call))
    else:
        call()
    sim.step_device(d_cmd.data_ptr(), 1)


def everybody():
    sim.observe_sparse_device(*lists)
    for k in range(2):
        full[k].predict_sparse(*lists, AGENTS, d_probs[k].data_ptr(), d_value[k].data_ptr(), d_cmds[k].data_ptr(), seed=100 + k,
                               reset_words=restarted)
    torch.where(d_owner, d_cmds[0], d_cmds[1], out=d_cmd)
    sim.step_device(d_cmd.data_ptr(), 1)


def one_network():
    sim.observe_sparse_device(*lists)
    full[0].predict_sparse(*lists, AGENTS, d_probs[0].data_ptr(), d_value[0].data_ptr(), d_cmd.data_ptr(), seed=100, reset_words=restarted)
    sim.step_device(d_cmd.data_ptr(), 1)


for i in range(WARM):
    (routed, everybody, one_network)[i % 3]()
series = {"routed": [], "everybody": [], "one_network": [], "routed_again": []}
for _ in range(REPS):
    series["routed"].append(span(routed))
    series["everybody"].append(span(everybody))
    series["one_network"].append(span(one_network))
    series["routed_again"].append(span(lambda: routed(timed=True)))
    gather_entries.append(torch.clamp(d_counts, max=CAP).to(torch.int64).sum())  # (read on the host after the series)
out = {"reps": REPS, "warmup": WARM, "unit": "ms, device events", "hbm_rate_TB_s": HBM_TBS, "workload": "C5", "arenas": ARENAS,
       "agents": AGENTS, "agents_per_network": [router.count(0), router.count(1)], "cap": CAP,
       "mean_list_entries": float(d_counts.float().mean().item()), "overflows": [p.sparse_overflows() for p in half + full]}
out.update({k: med(v) for k, v in series.items()})
out["gather_launch"], out["scatter_launch"] = med(gather_spans), med(scatter_spans)
# gather, per agent: the list entries (8 B each) and pov (640 B) read and written; the count read and written; (net, slot) 8 B;
# the restart word read, the flag byte written.  scatter (the command only), per agent: (net, slot) 8 B, one byte read and written
gb = float(np.median([int(n.item()) * 16 for n in gather_entries])) + AGENTS * (2 * 640 + 8 + 8 + 4 + 1)
sb = float(AGENTS * (8 + 2))
out["gather_bytes"], out["gather_bytes_over_hbm_rate_ms"] = gb, gb / (HBM_TBS * 1e12) * 1e3
out["scatter_bytes"], out["scatter_bytes_over_hbm_rate_ms"] = sb, sb / (HBM_TBS * 1e12) * 1e3
out["routed_over_everybody"] = out["routed"]["median"] / out["everybody"]["median"]
out["routed_minus_one_network_ms"] = out["routed"]["median"] - out["one_network"]["median"]
out["routed_again_over_routed"] = out["routed_again"]["median"] / out["routed"]["median"]
out["routed_is_shorter_than_everybody"] = bool(out["routed"]["median"] < out["everybody"]["median"])
for x in [router, sim] + half + full:
    x.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
