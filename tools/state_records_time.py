"""Device time of sf_state_device (k_state_init + k_state_records) on one MI355X, in one process.

    python tools/state_records_time.py [--arenas 4096] [--out profiles/state_records_time.json] [--no-policy-loop]
    python tools/state_records_time.py --host-digest-only          # with SF_LIBRARY_PATH: another build's host digest

Two worlds, 4096 arenas each, played 200 steps first: BASELINE configs[2] (64 x 64 cells, 8 / 24 / 64 / 8 slots) and the
reference's native dimensions (3 x 30 x 100 cells, pools of 64 / 9000 / 256 / 9000).  Four requests: the records of the four
tables; those and the three cell tables; the digest alone; everything.  Device events around the call alone, median of 21
after 10 warm-up calls.  For each: the bytes that must move (every packed word the decoder has to read once, every output
byte written once; the side tables of the cells are counted as not read: they are read only on player-built cells) and the
time those bytes take at the copy rate the project quotes (6.3 TB/s); the ratio is reported, not gated.  Beside it the wall time
of the host's sf_state_digest on the same state, and the policy loop of examples/policy_loop.py (4096 arenas, 200 steps) with
and without one state_records() call per step."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import abi, config, env

COPY_RATE = 6.3e12  # bytes/s: the device-to-device copy rate DESIGN.md quotes
WARMUP, REPEATS = 10, 21


def worlds(arenas):
    yield "configs[2]", config.baseline_workload("C3", arenas=arenas)
    cfg = config.make_config(arenas, 30, 100, floors=3, H=64, Z=9000, B=256, P=9000, mode=abi.MODE_TIMER, level=3)
    yield "native", config.Workload("native-9000", cfg, *config.three_floor_map(30, 100, wall_p=0.06, map_seed=11))


def played(w, steps=200):
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    cmds = torch.from_numpy(config.bench_commands(w.cfg.arenas, w.cfg.n_agents, steps)[0]).cuda()
    sim.step_device(cmds.data_ptr(), steps)
    sim.synchronize()
    return sim


def must_move(cfg, tables, cells, digest, rest):
    """(bytes read, bytes written) per arena of a request."""
    H, Z, B, P = cfg.cap_humans, cfg.cap_zombies, cfg.cap_bullets, cfg.cap_portals
    ncell = cfg.floors * cfg.rows * cfg.cols
    packed, records = 4 * (13 * H + 3 * Z + 4 * B + P), 4 * (28 * H + 7 * Z + 11 * B + 4 * P)
    rd = wr = 0
    if tables or digest or rest:  # (the counts walk the whole pools too)
        rd += packed
    if tables:
        wr += records
    if cells or digest:
        rd += ncell
    if cells:
        wr += 9 * ncell
    if digest or rest:
        rd += 4 * (24 + 18)
    if digest:
        wr += 8
    if rest:
        wr += 160 + 32
    return rd, wr


def time_request(sim, **kw):
    io, _ = sim.state_io(**kw)  # (tensors, struct and views are built here, once: the events see the launches alone)
    for _ in range(WARMUP):
        sim.state_device(io)
    sim.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sim.state_device(io)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def host_digest_ms(sim):
    sim.digest()
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        sim.digest()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def policy_loop(arenas, steps, with_records):
    from strikeforce_amd import policy
    w = config.baseline_workload("C2", arenas=arenas)
    sim = env.ArenaBatch(w)
    net = policy.PolicyBatch(policy.init_parameters(seed=0), arenas)
    stream = torch.cuda.Stream()
    cap = 2048
    with torch.cuda.stream(stream):
        sim.set_stream(stream.cuda_stream), net.set_stream(stream.cuda_stream)
        sim.reset(*w.seeds())
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        keys, vals, counts, pov = z((arenas, cap), torch.int32), z((arenas, cap), torch.float32), z(arenas, torch.int32), z((arenas, 160), torch.float32)
        dense = torch.empty((arenas, 32, 31, 31), dtype=torch.float32, device="cuda")
        probs, value, cmd = z((arenas, 9), torch.float32), z(arenas, torch.float32), z(arenas, torch.uint8)
        restarted = sim.done_view_device()

        def loop(n):
            for _ in range(n):
                sim.observe_sparse_device(keys.data_ptr(), vals.data_ptr(), counts.data_ptr(), pov.data_ptr(), cap)
                sim.observe_overflow_device(counts.data_ptr(), cap, dense.data_ptr(), pov.data_ptr())
                net.predict_sparse(keys.data_ptr(), vals.data_ptr(), counts.data_ptr(), pov.data_ptr(), cap, arenas, probs.data_ptr(),
                                   value.data_ptr(), cmd.data_ptr(), seed=1234, d_dense_ptr=dense.data_ptr(), reset_words=restarted)
                sim.step_device(cmd.data_ptr(), 1)
                if with_records:
                    sim.state_records(cells=True, digest=True)
            stream.synchronize()

        loop(20)
        t0 = time.perf_counter()
        loop(steps)
        dt = time.perf_counter() - t0
    sim.set_stream(None), net.set_stream(None)
    net.close(), sim.close()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-policy-loop", action="store_true")
    ap.add_argument("--host-digest-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    out = {"library": os.path.basename(env.LIB_PATH), "arenas": args.arenas, "copy_rate_bytes_per_s": COPY_RATE, "warmup": WARMUP, "repeats": REPEATS, "worlds": {}}
    requests = {"tables": dict(hdr=False, counts=False), "tables+cells": dict(hdr=False, counts=False, cells=True),
                "digest": dict(humans=0, zombies=0, bullets=0, portals=0, hdr=False, counts=False, digest=True),
                "everything": dict(cells=True, digest=True)}
    for name, w in worlds(args.arenas):
        sim = played(w)
        res = {"host_state_digest_ms": host_digest_ms(sim)}
        if not args.host_digest_only:
            assert np.array_equal(sim.digest_device().cpu().numpy().view(np.uint64), sim.digest())  # (what is timed is right)
            for rname, kw in requests.items():
                med, lo, hi = time_request(sim, **kw)
                rd, wr = must_move(w.cfg, "tables" in rname or rname == "everything", "cells" in rname or rname == "everything",
                                   rname in ("digest", "everything"), rname == "everything")
                total = (rd + wr) * args.arenas
                res[rname] = {"median_ms": med, "min_ms": lo, "max_ms": hi, "bytes_read": rd * args.arenas, "bytes_written": wr * args.arenas,
                              "ms_at_copy_rate": total / COPY_RATE * 1e3, "ratio_to_copy_rate": med / (total / COPY_RATE * 1e3)}
            res["host_over_device_digest"] = res["host_state_digest_ms"] / res["digest"]["median_ms"]
        out["worlds"][name] = res
        sim.close()
        print(name, json.dumps(res), flush=True)
    if not args.host_digest_only and not args.no_policy_loop:
        a, b, c = policy_loop(4096, 200, False), policy_loop(4096, 200, True), policy_loop(4096, 200, False)
        out["policy_loop_4096x200_s"] = {"without": [a, c], "with_state_records_everything": b}
        print("policy loop", json.dumps(out["policy_loop_4096x200_s"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
