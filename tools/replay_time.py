"""Per-iteration time of replaying logged matches, the lines fetched on the device against the lines fetched on the host.

    python tools/replay_time.py [--arenas 4096] [--rounds 3]

Every arena replays tests/golden/online_plain.sf_sample (a three-player match the reference's client logged, 120
iterations).  Device form: sf_replay_step per iteration (k_replay_fetch, k_step_half, k_replay_fetch, k_step_half), no host
synchronisation.  Host form, the only way before sf_replay_step: sf_step_begin, sf_agent_alive to the host, the lines
picked there (vectorised over the arenas), sf_step_end with a host command array.  Both end in the same digests
(asserted).  Prints one JSON line; the kernels' own times come from running this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from strikeforce_amd import config, env, replay  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    f = json.load(open(os.path.join(GOLDEN, "online_samples.json")))["matches"]["online_plain"]
    s = replay.read_sample(os.path.join(GOLDEN, f["file"]), layout="logged", teams=f["teams"])
    m = f["map"]
    chars, portal = config.synthetic_map(m["rows"], m["cols"], wall_p=m["wall_p"], portal_pairs=m["portal_pairs"])
    A, n, ind, iters = args.arenas, s.players, s.ind, f["iterations"]
    sim = env.ArenaBatch(replay.workload_for(s, m["rows"], m["cols"], chars, portal, arenas=A, **f["pools"]))
    tb, sr = (C.c_uint64 * A)(*[s.tb] * A), (C.c_uint64 * A)(*[s.serial] * A)
    tok = np.frombuffer(s.commands.encode(), dtype=np.uint8)
    rows = np.arange(A)
    dev, host = [], []
    for _ in range(args.rounds):
        sim.reset(tb, sr)
        sim.replay_load([s] * A)
        sim.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            sim.replay_step()
        sim.synchronize()
        dev.append((time.perf_counter() - t) / iters)
        want = sim.digest()
        sim.replay_load(None)
        sim.reset(tb, sr)
        cur = np.zeros(A, dtype=np.int64)
        sim.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            cmd = np.full((A, n), ord("+"), dtype=np.uint8)
            cmd[:, ind] = tok[cur]
            cur += 1
            sim.step_begin()
            alive = sim.agent_alive()
            for g in range(n):
                if g == ind:
                    continue
                take = alive[:, g] != 0
                cmd[take, g] = tok[cur[take]]
                cur[take] += 1
            sim.step_end(cmd)
        sim.synchronize()
        host.append((time.perf_counter() - t) / iters)
        assert (sim.digest() == want).all() and (cur == len(tok)).all()
    print(json.dumps({"arenas": A, "iterations": iters, "players": n,
                      "device_fetch_us_per_iteration": round(1e6 * min(dev), 1),
                      "host_fetch_us_per_iteration": round(1e6 * min(host), 1),
                      "all_rounds_us": {"device": [round(1e6 * x, 1) for x in dev], "host": [round(1e6 * x, 1) for x in host]}}))


if __name__ == "__main__":
    main()
