"""Cost of the episode log on the step loop (strikeforce.h sf_episode_log), in one process on one card.

    python tools/episode_log_ab.py [--arenas 4096] [--k 20] [--launches 300] [--workloads C3 C2]

For each workload: the same k-step launch loop (sf_step_device on random-action commands) with the log off,
and with the log on (depth 8) plus one sf_episodes_device per launch — the loop a training run would capture.  Prints one
JSON line per workload: env-steps/s of both, their ratio, and records collected per launch.  The two loops alternate
in rounds so that clock drift hits both alike.  The collection kernels' own time comes from running this under
`rocprofv3 --kernel-trace --stats` (k_ep_plan, k_ep_copy)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from strikeforce_amd import config, env  # noqa: E402


def loop(g, d, k, launches, out=None, counts=None, max_records=0):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(launches):
        g.step_device(d[(i * k) % (d.shape[0] - k + 1)].data_ptr(), k)
        if out is not None:
            g.episodes_device(out.data_ptr(), max_records, counts.data_ptr())
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--workloads", nargs="+", default=["C3", "C2"])
    a = ap.parse_args()
    for wl in a.workloads:
        w = config.baseline_workload(wl, arenas=a.arenas)
        off, on = env.ArenaBatch(w), env.ArenaBatch(w)
        on.enable_episode_log(a.depth)
        tb, sr = w.seeds()
        off.reset(tb, sr), on.reset(tb, sr)
        cmds, _ = config.bench_commands(a.arenas, w.cfg.n_agents, 2000)
        d = torch.from_numpy(cmds).cuda()
        cap = a.arenas * a.depth
        out = torch.zeros((cap, on.episode_record_words), dtype=torch.int32, device="cuda")
        counts = torch.zeros(3, dtype=torch.int32, device="cuda")
        loop(off, d, a.k, 20), loop(on, d, a.k, 20, out, counts, cap)  # warm-up (and past the first episode ends)
        t_off = t_on = 0.0
        last = []  # records the last collection of each round delivered
        for _ in range(a.rounds):
            t_off += loop(off, d, a.k, a.launches)
            t_on += loop(on, d, a.k, a.launches, out, counts, cap)
            last.append(int(counts[0]))
        steps = a.rounds * a.launches * a.k * a.arenas
        print(json.dumps({"workload": wl, "arenas": a.arenas, "k": a.k, "depth": a.depth,
                          "off_steps_per_s": steps / t_off, "on_steps_per_s": steps / t_on,
                          "on_over_off": t_off / t_on, "records_per_collection": last}), flush=True)
        off.close(), on.close()


if __name__ == "__main__":
    main()
