"""What sf_reset_arenas costs ("Restart of chosen arenas"), one process:

    python tools/reset_sel_time.py [out.json]        (default profiles/reset_sel_time.json)

BASELINE configs[2] at 4096 arenas; device events unless said otherwise; medians of 21 after 10 warm-ups; the variants
alternate inside one run.
(a) the launch with nothing chosen, beside the interactive tick it would join (observe_sparse -> predict_sparse -> one step):
    ticks alternate without / with / without the call; the second without-series gives the spread between two identical
    series.  Also the launch alone.
(b) all arenas chosen with the seeds on the device, against sf_reset: wall time of call + synchronise for both (sf_reset
    ends in a synchronisation of its own), and the k_reset_sel launch alone by device events.
(c) examples/eval_fixed_seeds.py 4096 4 against the same number of rounds of whole-batch sf_reset: agent-steps/s of arenas
    whose game is running, games finished and cut, for both, and for the example calling every 8th tick only; the same
    three with a step limit of 1000.
Prints one JSON object."""
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from strikeforce_amd import config, env, policy

REPS, WARM, CAP, ARENAS = 21, 10, 2048, 4096
out = {"reps": REPS, "warmups": WARM, "arenas": ARENAS, "config": "configs[2]"}


def span(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def med_events(pairs):
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in pairs])
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}


def med_wall(ts):
    t = np.array(ts) * 1e3
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}


w = config.baseline_workload("C3", arenas=ARENAS)
assert w.cfg.n_agents == 1
sim = env.ArenaBatch(w)
tb, sr = w.seeds()
sim.reset(tb, sr)
net = policy.PolicyBatch(policy.init_parameters(seed=0), ARENAS)
i32 = dict(dtype=torch.int32, device="cuda")
d_keys, d_counts = torch.zeros((ARENAS, CAP), **i32), torch.zeros(ARENAS, **i32)
d_vals, d_pov = torch.zeros((ARENAS, CAP), device="cuda"), torch.zeros((ARENAS, 160), device="cuda")
d_probs, d_value = torch.zeros((ARENAS, 9), device="cuda"), torch.zeros(ARENAS, device="cuda")
d_cmd = torch.zeros(ARENAS, dtype=torch.uint8, device="cuda")
d_none = torch.zeros(ARENAS, dtype=torch.uint8, device="cuda")
d_all = torch.ones(ARENAS, dtype=torch.uint8, device="cuda")
d_sel = torch.zeros(ARENAS, dtype=torch.uint8, device="cuda")
d_tb = torch.from_numpy(np.array(list(tb), dtype=np.uint64).view(np.int64)).cuda()
d_sr = torch.from_numpy(np.array(list(sr), dtype=np.uint64).view(np.int64)).cuda()
restarted = sim.done_view_device()
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
none_chosen = lambda: sim.reset_arenas(mask_ptr=d_none.data_ptr(), tb_ptr=d_tb.data_ptr(), serial_ptr=d_sr.data_ptr(),
                                       selected_ptr=d_sel.data_ptr())
launch_spans = []


def tick(with_call, timed=False):
    if with_call:
        if timed:
            launch_spans.append(span(none_chosen))
        else:
            none_chosen()
    sim.observe_sparse_device(*lists)
    net.predict_sparse(*lists, ARENAS, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=7, reset_words=restarted)
    sim.step_device(d_cmd.data_ptr(), 1)


# ---- (a) nothing chosen, beside the interactive tick ----------------------------------------------------------------------
for i in range(WARM):
    tick(i % 2 == 1)
series = {"without": [], "with": [], "without_again": []}
for _ in range(REPS):
    series["without"].append(span(lambda: tick(False)))
    series["with"].append(span(lambda: tick(True, timed=True)))
    series["without_again"].append(span(lambda: tick(False)))
row = {k: med_events(v) for k, v in series.items()}
row["launch_alone"] = med_events(launch_spans)
row["with_minus_without_ms"] = row["with"]["median_ms"] - row["without"]["median_ms"]
row["without_again_over_without"] = row["without_again"]["median_ms"] / row["without"]["median_ms"]
assert int(d_sel.sum().item()) == 0
out["nothing_chosen"] = row

# ---- (b) everything chosen, seeds on the device, against sf_reset ---------------------------------------------------------------
all_chosen = lambda: sim.reset_arenas(mask_ptr=d_all.data_ptr(), tb_ptr=d_tb.data_ptr(), serial_ptr=d_sr.data_ptr(),
                                      selected_ptr=d_sel.data_ptr())


def wall(fn):
    sim.synchronize()
    t0 = time.perf_counter()
    fn()
    sim.synchronize()
    return time.perf_counter() - t0


walls = {"sf_reset": [], "sf_reset_arenas": [], "sf_reset_again": []}
kernel_spans = []
for i in range(WARM + REPS):
    a = wall(lambda: sim.reset(tb, sr))
    b = wall(all_chosen)
    c = wall(lambda: sim.reset(tb, sr))
    k = span(all_chosen)
    if i >= WARM:
        walls["sf_reset"].append(a), walls["sf_reset_arenas"].append(b), walls["sf_reset_again"].append(c), kernel_spans.append(k)
row = {k: med_wall(v) for k, v in walls.items()}
row["unit"] = "wall ms, call + synchronise"
row["k_reset_sel_launch_device"] = med_events(kernel_spans)
row["reset_arenas_over_reset"] = row["sf_reset_arenas"]["median_ms"] / row["sf_reset"]["median_ms"]
row["reset_again_over_reset"] = row["sf_reset_again"]["median_ms"] / row["sf_reset"]["median_ms"]
assert int(d_sel.sum().item()) == ARENAS
out["all_chosen"] = row
net.close(), sim.close()

# ---- (c) the example against whole-batch rounds ---------------------------------------------------------------------------------
spec = importlib.util.spec_from_file_location("eval_fixed_seeds", os.path.join(ROOT, "examples", "eval_fixed_seeds.py"))
ex = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ex)
GAMES, MAX_STEPS = 4, 200
ex.run(256, 1, 20), ex.run(256, 1, 20, whole_batch=True)  # (warm-up: allocations, first launches)
out["eval_fixed_seeds"] = {"per_arena_restarts": ex.run(ARENAS, GAMES, MAX_STEPS),
                           "per_arena_restarts_every_8_ticks": ex.run(ARENAS, GAMES, MAX_STEPS, restart_every=8),
                           "whole_batch_rounds": ex.run(ARENAS, GAMES, MAX_STEPS, whole_batch=True)}
# the same with a limit most games end before (configs[1]: a game lasts some hundred steps): finished arenas stand still longer
out["eval_fixed_seeds_limit_1000"] = {"per_arena_restarts": ex.run(ARENAS, GAMES, 1000),
                                      "per_arena_restarts_every_8_ticks": ex.run(ARENAS, GAMES, 1000, restart_every=8),
                                      "whole_batch_rounds": ex.run(ARENAS, GAMES, 1000, whole_batch=True)}
print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reset_sel_time.json")
json.dump(out, open(path, "w"), indent=1)
