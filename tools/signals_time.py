"""What sf_signals_step costs ("Per-step signals"), at 4096 arenas of BASELINE configs[1] and configs[2].

    python tools/signals_time.py kernels                    the launches to look at under a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/signals_time.py kernels
      per configuration 50 steps, then 40 rounds of sf_done_device, sf_agent_alive_device and sf_signals_step with all three
      outputs, a step between the rounds.  k_done and k_agent_alive have one lane per (arena, agent) and touch the same rows:
      they are the yardstick.
    python tools/signals_time.py loop [label]               one JSON line: the rate of examples/policy_loop.py's loop
      (observe_sparse -> predict_sparse -> step) in series of 200 ticks that alternate without / with the call / without
      again, medians of 5 series each; the second without-series gives the spread between two identical series.  With
      SF_LIBRARY_PATH set to another build of the library (the parent commit's) that has no sf_signals_*, only the
      without-series run: the parent's rate from the same session.
    python tools/signals_time.py merge DIR LOOP.json PARENT.json [out.json]
      the kernel statistics of DIR, the two loop lines, the ratios and the bytes per agent into profiles/signals_time.json."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARENAS, CAP = 4096, 2048
CONFIGS = (("configs[1]", "C2"), ("configs[2]", "C3"))
# what one lane of k_signals moves: 8 words of the human row, 11 of the scalar block, the latch row (8), the baseline row
# read (16) and written (15), the outputs (16 + 8 + 1); the scalar block's 64-byte lines are shared by an arena's agents
BYTES_PER_AGENT = {"read": 4 * (8 + 11 + 8 + 16), "written_baseline": 4 * 15, "written_outputs": 4 * (16 + 8 + 1)}


def kernels():
    import torch
    from strikeforce_amd import abi, config, env
    for key, which in CONFIGS:
        w = config.baseline_workload(which, arenas=ARENAS)
        n = w.cfg.n_agents
        sim = env.ArenaBatch(w)
        sim.reset(*w.seeds())
        cmds, _ = config.bench_commands(ARENAS, n, 50 + 40)
        d_cmds = torch.from_numpy(cmds).cuda()
        sim.step_device(d_cmds.data_ptr(), 50)
        sig = sim.signals()
        v = torch.zeros((ARENAS, n, abi.VITALS_WORDS), dtype=torch.int32, device="cuda")
        d = torch.zeros((ARENAS, n, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
        r = torch.zeros(ARENAS * n, dtype=torch.float32, device="cuda")
        flags = torch.zeros(ARENAS * n, dtype=torch.uint8, device="cuda")
        wts = env.reward_weights(per_step=-0.01, kills=1.0, hp=0.01, died=-1.0, outcome=[0, -1, 2, -1, 1, 0, 0, 0])
        for s in range(40):
            sim.step_device(d_cmds[50 + s].data_ptr(), 1)
            sim.done_device(flags.data_ptr())
            sim.agent_alive_device(flags.data_ptr())
            sig.step(v, d, r, None, wts)
        sim.synchronize()
        assert sig.status()[1] == 0
        sig.close(), sim.close()


def loop(label):
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
    d_reward = torch.zeros(agents, dtype=torch.float32, device="cuda")
    restarted = sim.done_view_device()
    has = hasattr(sim.L, "sf_signals_create")
    sig = sim.signals() if has else None
    wts = env.reward_weights(per_step=-0.01, kills=1.0, hp=0.01, died=-1.0, outcome=[0, -1, 2, -1, 1, 0, 0, 0]) if has else None

    def series(with_call, ticks=200):
        sim.synchronize(), net.synchronize()
        t0 = time.perf_counter()
        for _ in range(ticks):
            sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
            sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
            net.predict_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, agents, d_probs.data_ptr(),
                               d_value.data_ptr(), d_cmd.data_ptr(), seed=1234, d_dense_ptr=d_dense.data_ptr(), reset_words=restarted)
            sim.step_device(d_cmd.data_ptr(), 1)
            if with_call:
                sig.step(reward_ptr=d_reward, weights=wts)
        sim.synchronize(), net.synchronize()
        return agents * ticks / (time.perf_counter() - t0) / 1e6

    kinds = {"without": False, "with_signals": True, "without_again": False} if has else {"without": False, "without_again": False}
    series(False), series(has)  # warm-up
    rates = {k: [] for k in kinds}
    for _ in range(5):
        for k, flag in kinds.items():
            rates[k].append(series(flag))
    out = {"label": label, "arenas": ARENAS, "ticks_per_series": 200, "series": 5, "library_has_signals": has,
           "M_agent_steps_per_s": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in rates.items()}}
    print(json.dumps(out))


def merge(directory, loop_json, parent_json, path):
    rows = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for k in ("k_signals", "k_done", "k_agent_alive"):
                if k + "(" in row["Name"]:
                    rows[k] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]), "min_ns": int(row["MinNs"]),
                               "max_ns": int(row["MaxNs"])}
    out = {"arenas": ARENAS, "configurations": [k for k, _ in CONFIGS],
           "kernel_trace": rows, "bytes_per_agent": dict(BYTES_PER_AGENT, total=sum(BYTES_PER_AGENT.values())),
           "note": "kernel statistics are over both configurations' launches (4096 and 4096 lanes: one commanded human each)"}
    if "k_signals" in rows:
        out["ratio_to_k_done"] = rows["k_signals"]["average_ns"] / rows["k_done"]["average_ns"]
        out["ratio_to_k_agent_alive"] = rows["k_signals"]["average_ns"] / rows["k_agent_alive"]["average_ns"]
    last = lambda f: json.loads([line for line in open(f) if line.startswith("{")][-1])
    out["policy_loop"], out["policy_loop_parent_library"] = last(loop_json), last(parent_json)
    m = out["policy_loop"]["M_agent_steps_per_s"]
    out["with_over_without"] = m["with_signals"]["median"] / m["without"]["median"]
    out["without_again_over_without"] = m["without_again"]["median"] / m["without"]["median"]
    out["without_over_parent_without"] = m["without"]["median"] / out["policy_loop_parent_library"]["M_agent_steps_per_s"]["without"]["median"]
    print(json.dumps(out))
    json.dump(out, open(path, "w"), indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels()
    elif mode == "loop":
        loop(sys.argv[2] if len(sys.argv) > 2 else "this build")
    elif mode == "merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "signals_time.json"))
    else:
        sys.exit(__doc__)
