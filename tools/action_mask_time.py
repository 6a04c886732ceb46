"""What sf_action_mask_device costs ("Action masks"), at 4096 arenas.

    python tools/action_mask_time.py kernels WHICH          the launches to look at under a kernel trace, one run per WHICH
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/action_mask_time.py kernels configs1
      WHICH: configs1 (BASELINE configs[1], 1 agent), configs2 (configs[2]), battle8 (an 8-agent 256 x 256 Battle).  50 steps,
      then 40 rounds of sf_observe_sparse_device, sf_signals_step and sf_action_mask_device (command words and the bots' action
      words), a step between the rounds.  The list observation's launch is the yardstick: the mask reads a small part of what
      that kernel reads.
    python tools/action_mask_time.py loop                   one JSON line: the rate of examples/policy_loop.py's loop
      (observe_sparse -> predict_sparse -> step) and of examples/masked_policy_loop.py's (observe_sparse -> reset_memory ->
      forward_sparse -> action_mask -> act_masked -> step) and of the latter with the unmasked draw, in series of 200 ticks
      that alternate, medians of 5 series each; the plain loop runs twice per round, which gives the spread between two
      identical series.  Also the share of drawn commands that were effective with and without the mask.
    python tools/action_mask_time.py merge DIR1 DIR2 DIR8 LOOP.json [out.json]
      the kernel statistics of the three traces, the loop line and the ratios into profiles/action_mask_time.json."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARENAS, CAP = 4096, 2048
KERNELS = ("k_action_mask", "k_signals", "k_observe_list")


def workload(which):
    from strikeforce_amd import abi, config
    if which == "configs1":
        return config.baseline_workload("C2", arenas=ARENAS)
    if which == "configs2":
        return config.baseline_workload("C3", arenas=ARENAS)
    if which == "battle8":  # BASELINE configs[4]'s world: 256 x 256, Battle, 8 commanded humans
        return config.baseline_workload("C5", arenas=ARENAS)
    raise ValueError(which)


def kernels(which):
    import torch
    from strikeforce_amd import abi, config, env
    w = workload(which)
    n = w.cfg.n_agents
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    cmds, _ = config.bench_commands(ARENAS, n, 50 + 40)
    d_cmds = torch.from_numpy(cmds).cuda()
    sim.step_device(d_cmds.data_ptr(), 50)
    sig = sim.signals()
    agents = ARENAS * n
    v = torch.zeros((ARENAS, n, abi.VITALS_WORDS), dtype=torch.int32, device="cuda")
    d = torch.zeros((ARENAS, n, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
    r = torch.zeros(agents, dtype=torch.float32, device="cuda")
    d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
    d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
    d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
    wts = env.reward_weights(per_step=-0.01, kills=1.0, hp=0.01, died=-1.0, outcome=[0, -1, 2, -1, 1, 0, 0, 0])
    for s in range(40):
        sim.step_device(d_cmds[50 + s].data_ptr(), 1)
        sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
        sig.step(v, d, r, None, wts)
        sim.action_mask("+xzqeawsd")
    sim.synchronize()
    sig.close(), sim.close()


def loop():
    import numpy as np
    import torch
    from strikeforce_amd import config, env, policy
    w = config.baseline_workload("C2", arenas=ARENAS)
    sim = env.ArenaBatch(w)
    agents = ARENAS * w.cfg.n_agents
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
    restarted = sim.done_view_device()
    effective = {k: torch.zeros((), dtype=torch.int64, device="cuda") for k in ("masked_loop", "masked_loop_unmasked_draw")}
    ticks_of = dict.fromkeys(effective, 0)

    def series(kind, ticks=200):
        sim.synchronize(), net.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
            sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
            if kind.startswith("policy_loop"):
                net.predict_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, agents,
                                   d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=1234, d_dense_ptr=d_dense.data_ptr(),
                                   reset_words=restarted)
            else:
                sim.done_device(d_done.data_ptr())
                net.reset_memory(d_done.data_ptr(), agents)
                net.forward_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, agents,
                                   d_probs.data_ptr(), d_value.data_ptr(), d_dense_ptr=d_dense.data_ptr())
                _, actions = sim.action_mask(policy.ACTION_STRING)
                if kind == "masked_loop":
                    net.act_masked(d_probs.data_ptr(), agents, actions.data_ptr(), d_cmd.data_ptr(), seed=1234,
                                   d_action_ptr=d_action.data_ptr())
                else:
                    net.act(d_probs.data_ptr(), agents, d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr())
            sim.step_device(d_cmd.data_ptr(), 1)
        sim.synchronize(), net.synchronize()
        rate = agents * ticks / (time.perf_counter() - t0) / 1e6
        if kind in effective:  # one more tick outside the timed window, with the bookkeeping: what share of the draws was effective
            for _ in range(20):
                sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
                sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
                net.forward_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, agents,
                                   d_probs.data_ptr(), d_value.data_ptr(), d_dense_ptr=d_dense.data_ptr())
                _, actions = sim.action_mask(policy.ACTION_STRING)
                if kind == "masked_loop":
                    net.act_masked(d_probs.data_ptr(), agents, actions.data_ptr(), d_cmd.data_ptr(), seed=99, d_action_ptr=d_action.data_ptr())
                else:
                    net.act(d_probs.data_ptr(), agents, d_cmd.data_ptr(), seed=99, d_action_ptr=d_action.data_ptr())
                effective[kind] += ((actions.reshape(-1) >> d_action) & 1).sum()
                sim.step_device(d_cmd.data_ptr(), 1)
            ticks_of[kind] += 20
        return rate

    kinds = ("policy_loop", "masked_loop", "masked_loop_unmasked_draw", "policy_loop_again")
    for k in kinds:
        series(k, 50)  # warm-up
    rates = {k: [] for k in kinds}
    for _ in range(5):
        for k in kinds:
            rates[k].append(series(k))
    out = {"arenas": ARENAS, "configuration": "configs[1]", "ticks_per_series": 200, "series": 5,
           "M_agent_steps_per_s": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in rates.items()},
           "share_of_draws_effective": {k: float(effective[k].item()) / (agents * ticks_of[k]) for k in effective}}
    print(json.dumps(out))


def merge(dirs, loop_json, path):
    out = {"arenas": ARENAS, "kernel_trace": {}}
    for which, directory in zip(("configs1", "configs2", "battle8"), dirs):
        rows = {}
        for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k + "(" in row["Name"] or k + "<" in row["Name"]:
                        rows[k] = {"name": row["Name"][:60], "calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                   "min_ns": int(row["MinNs"]), "max_ns": int(row["MaxNs"])}
        if "k_action_mask" in rows and "k_observe_list" in rows:
            rows["mask_over_observe_list"] = rows["k_action_mask"]["average_ns"] / rows["k_observe_list"]["average_ns"]
        if "k_action_mask" in rows and "k_signals" in rows:
            rows["mask_over_signals"] = rows["k_action_mask"]["average_ns"] / rows["k_signals"]["average_ns"]
        out["kernel_trace"][which] = rows
    last = lambda f: json.loads([line for line in open(f) if line.startswith("{")][-1])
    out["loops"] = last(loop_json)
    m = out["loops"]["M_agent_steps_per_s"]
    out["masked_over_policy_loop"] = m["masked_loop"]["median"] / m["policy_loop"]["median"]
    out["policy_loop_again_over_policy_loop"] = m["policy_loop_again"]["median"] / m["policy_loop"]["median"]
    print(json.dumps(out))
    json.dump(out, open(path, "w"), indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels" and len(sys.argv) > 2:
        kernels(sys.argv[2])
    elif mode == "loop":
        loop()
    elif mode == "merge" and len(sys.argv) > 5:
        merge(sys.argv[2:5], sys.argv[5], sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "action_mask_time.json"))
    else:
        sys.exit(__doc__)
