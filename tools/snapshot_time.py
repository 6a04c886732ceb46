"""What sf_snapshot_save / sf_snapshot_load cost ("Arena snapshots"), one process:

    python tools/snapshot_time.py [out.json]        (default profiles/snapshot_time.json)

4096 arenas; device events; medians of 21 after 10 warm-ups; the variants alternate inside one run.
(a) save and load of all arenas of BASELINE configs[2] and of configs[4] (256 x 256, the flag plane in HBM), each beside two
    yardsticks: the bytes the call must move (every slot byte read once and written once) at the 6.29 TB/s the
    micro-architecture guide measured for a float4 copy, and hipMemcpyDtoDAsync of the same number of bytes in one piece.
(b) a load that names one arena, and a call that names none: the cost of the launch alone.
(c) one tick of the interactive loop (observe_sparse -> predict_sparse -> step) without, with and without again a save of
    every arena; the second without-series gives the spread between two identical series.
Prints one JSON object."""
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from strikeforce_amd import config, env, policy

REPS, WARM, CAP, ARENAS = 21, 10, 2048, 4096
COPY_RATE = 6.29e12  # bytes/s read + written, float4 copy (MI355X micro-architecture guide)
out = {"reps": REPS, "warmups": WARM, "arenas": ARENAS, "guide_copy_rate_bytes_per_s": COPY_RATE}

lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
H = C.CDLL(lib[0] if lib else "libamdhip64.so")
H.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


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


def alternate(variants):
    """{name: fn} -> {name: stats}: WARM rounds untimed, then REPS rounds, the variants taking turns inside each round."""
    for _ in range(WARM):
        for fn in variants.values():
            fn()
    spans = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            spans[k].append(span(fn))
    return {k: med_events(v) for k, v in spans.items()}


i32 = dict(dtype=torch.int32, device="cuda")
d_all = torch.arange(ARENAS, **i32)
d_none = torch.full((ARENAS,), -1, **i32)
d_one = d_none.clone()
d_one[ARENAS // 2] = 7

for key, which in (("configs[2]", "C3"), ("configs[4]", "C5")):
    w = config.baseline_workload(which, arenas=ARENAS)
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    cmds, _ = config.bench_commands(ARENAS, w.cfg.n_agents, 50)
    d_cmds = torch.from_numpy(cmds).cuda()
    sim.step_device(d_cmds.data_ptr(), 50)
    sim.synchronize()
    device_bytes, blob_bytes = sim.snapshot_slot_bytes()
    snap = sim.snapshot(ARENAS)
    moved = 2 * (device_bytes - 4) * ARENAS  # read once, written once
    src = torch.zeros((device_bytes - 4) * ARENAS, dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    snap.save(d_all)
    row = alternate({
        "save_all": lambda: snap.save(d_all),
        "load_all": lambda: snap.load(d_all),
        "memcpy_dtod_one_piece": lambda: H.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), src.numel(), None),
    })
    row["slot_bytes"] = device_bytes - 4
    row["bytes_moved"] = moved
    row["at_guide_copy_rate_ms"] = moved / COPY_RATE * 1e3
    for k in ("save_all", "load_all", "memcpy_dtod_one_piece"):
        row[k]["bytes_per_s"] = moved / (row[k]["median_ms"] * 1e-3)
    if key == "configs[2]":
        # ---- (b) the launch alone ------------------------------------------------------------------------------------------------
        out["one_arena_and_none"] = alternate({
            "load_one_arena": lambda: snap.load(d_one),
            "load_none": lambda: snap.load(d_none),
            "save_none": lambda: snap.save(d_none),
        })
        # ---- (c) beside the interactive tick ---------------------------------------------------------------------------------------
        assert w.cfg.n_agents == 1
        net = policy.PolicyBatch(policy.init_parameters(seed=0), ARENAS)
        d_keys, d_counts = torch.zeros((ARENAS, CAP), **i32), torch.zeros(ARENAS, **i32)
        d_vals, d_pov = torch.zeros((ARENAS, CAP), device="cuda"), torch.zeros((ARENAS, 160), device="cuda")
        d_probs, d_value = torch.zeros((ARENAS, 9), device="cuda"), torch.zeros(ARENAS, device="cuda")
        d_cmd = torch.zeros(ARENAS, dtype=torch.uint8, device="cuda")
        restarted = sim.done_view_device()
        lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)

        def tick(with_save):
            if with_save:
                snap.save(d_all)
            sim.observe_sparse_device(*lists)
            net.predict_sparse(*lists, ARENAS, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=7, reset_words=restarted)
            sim.step_device(d_cmd.data_ptr(), 1)

        t = alternate({"without": lambda: tick(False), "with_save_all": lambda: tick(True), "without_again": lambda: tick(False)})
        t["with_minus_without_ms"] = t["with_save_all"]["median_ms"] - t["without"]["median_ms"]
        t["without_again_minus_without_ms"] = t["without_again"]["median_ms"] - t["without"]["median_ms"]
        out["interactive_tick"] = t
        net.close()
    assert snap.status() == (0, 0)
    out[key] = row
    snap.close(), sim.close()
    del src, dst

print(json.dumps(out))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snapshot_time.json")
json.dump(out, open(path, "w"), indent=1)
