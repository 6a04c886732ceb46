"""What recording costs per iteration on one MI355X, in one process.

    python tools/record_step_time.py [--arenas 4096] [--out profiles/record_step_time.json]
    SF_LIBRARY_PATH=<another build> python tools/record_step_time.py --tag parent      # that build's step and split step

Two worlds, 4096 arenas each: BASELINE configs[2] (64 x 64 cells, one player) and the three-player Battle of
tests/online_cases.BATCH (28 x 36 cells, H 12, Z 10, B 48, P 48), both under auto_reset with the random-action commands of
the benchmark.  Per world the wall time per iteration, on a stream of the library's own, of
    step     sf_step_device(d_cmd, 1)
    split    sf_step_begin + sf_step_end_device
    record   sf_record_step
    collect  sf_record_step with sf_record_collect_device every 64 iterations
each over 256 iterations between two synchronisations, median of 7 runs after one warm-up run.  A build without
sf_record_* (the parent's, through SF_LIBRARY_PATH) gives the first two; --tag says under which name the figures go into the
JSON, which is read and extended, so that both builds end up in one file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import abi, config, env, replay

ITERS, RUNS, EVERY = 256, 7, 64
RECORD = [15000, 1000, 15000, 1, 1, 1, 300000, 60, 0, 0, 0, 1, 1, 1, 34] + [1] * 16 + [56]


def worlds(arenas):
    yield "configs[2]", config.baseline_workload("C3", arenas=arenas)
    proto = replay.Sample(1, 2, RECORD, "", name="p1", ind=1, team=2, players=3, names=["p0", "p1", "p2"], records=[RECORD] * 3,
                          teams=[1, 2, 3])
    chars, portal = config.synthetic_map(28, 36, wall_p=0.04, portal_pairs=1)
    w = replay.workload_for(proto, 28, 36, chars, portal, arenas=arenas, H=12, Z=10, B=48, P=48)
    w.cfg.auto_reset = 1
    yield "batch", w


def timed(sim, w, body, before=None):
    """every run plays the same ITERS iterations from the reset on"""
    us = []
    for run in range(RUNS + 1):
        sim.reset(*w.seeds())
        if before:
            before()
        sim.synchronize()
        t0 = time.perf_counter()
        for t in range(ITERS):
            body(t)
        sim.synchronize()
        if run:
            us.append((time.perf_counter() - t0) / ITERS * 1e6)
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))


def measure(w):
    sim = env.ArenaBatch(w)
    stream = torch.cuda.Stream()
    sim.set_stream(stream.cuda_stream)
    A, n = w.cfg.arenas, w.cfg.n_agents
    cmds = torch.from_numpy(config.bench_commands(A, n, ITERS)[0]).cuda()
    torch.cuda.synchronize()
    out = {"step": timed(sim, w, lambda t: sim.step_device(cmds[t].data_ptr(), 1))}

    def split(t):
        sim.step_begin()
        sim.step_end_device(cmds[t].data_ptr())
    out["split"] = timed(sim, w, split)
    if hasattr(sim.L, "sf_record_create"):
        bpa, G = n * (ITERS + 1), 64
        rec = sim.recorder(bpa, G)
        d_bytes = torch.zeros(A * bpa, dtype=torch.uint8, device="cuda")
        d_games = torch.zeros((A * G, abi.RECORD_GAME_WORDS), dtype=torch.int32, device="cuda")
        d_counts = torch.zeros(abi.RECORD_COUNT_WORDS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def empty():  # (an empty recorder in front of every run: the games of the run before are thrown away)
            rec.flush()
            rec.collect_device(d_bytes, A * bpa, d_games, A * G, d_counts)
        out["record"] = timed(sim, w, lambda t: rec.step(cmds[t]), before=empty)

        def collect(t):
            rec.step(cmds[t])
            if t % EVERY == EVERY - 1:
                rec.collect_device(d_bytes, A * bpa, d_games, A * G, d_counts)
        out["collect"] = timed(sim, w, collect, before=empty)
        out["collect"]["last_counts"] = dict(zip(abi.RECORD_COUNT_FIELDS, d_counts.cpu().tolist()))
        for k in ("record", "collect"):
            out[k]["over_split_us"] = round(out[k]["median_us"] - out["split"]["median_us"], 2)
        rec.close()
    sim.set_stream(0)
    sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--tag", default="branch")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "record_step_time.json"))
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(device=torch.cuda.get_device_name(0), arenas=a.arenas, iterations=ITERS, runs=RUNS, collect_every=EVERY,
               unit="microseconds of wall time per iteration, median of the runs")
    doc[a.tag] = {name: measure(w) for name, w in worlds(a.arenas)}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc[a.tag], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
