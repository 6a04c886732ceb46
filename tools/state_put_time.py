"""Device time of sf_state_put_device (k_put_init + k_put_check + k_put_write) on one MI355X, in one process, beside two
yardsticks measured in the same process.

    python tools/state_put_time.py [--arenas 4096] [--out profiles/state_put_time.json]

Two worlds, 4096 arenas each, played 200 steps first: BASELINE configs[2] and the reference's native dimensions (3 x 30 x 100
cells, pools of 64 / 9000 / 256 / 9000), as tools/state_records_time.py has them.  The put takes what sf_state_device wrote
for all arenas (header, four tables, three cell tables; row a -> arena a).  Yardsticks: sf_state_device with the four tables
and the cells and no digest (the same bytes in the other direction), and sf_snapshot_load of all arenas.  Device events around
the calls alone; two series of the put and two of each yardstick, alternating with the order rotating; medians of 21 after 10
warm-up calls.  A yardstick's spread is the difference of its two medians.  Reported, not gated: whether the put takes no more
than twice the sf_state_device median plus that spread (it reads its records twice — check, then write — and writes the
packed state once), the bytes that must move and those bytes at the copy rate the project quotes (6.3 TB/s)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (tools/state_records_time.py: the worlds and the constants)
import numpy as np
import torch

from strikeforce_amd import env
from state_records_time import COPY_RATE, REPEATS, WARMUP, played, worlds


def series(call, sync):
    for _ in range(WARMUP):
        call()
    sync()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def must_move(cfg):
    """(bytes the put reads, bytes it writes) per arena: the records twice, the packed state once."""
    H, Z, B, P = cfg.cap_humans, cfg.cap_zombies, cfg.cap_bullets, cfg.cap_portals
    ncell = cfg.floors * cfg.rows * cfg.cols
    records = 160 + 4 * (28 * H + 7 * Z + 11 * B + 4 * P) + 9 * ncell
    packed = 4 * (13 * H + 3 * Z + 4 * B + P) + ncell + 4 * (24 + 18 + 18)  # (the side tables only on player-built cells)
    return 2 * records, packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    out = {"library": os.path.basename(env.LIB_PATH), "arenas": args.arenas, "copy_rate_bytes_per_s": COPY_RATE, "warmup": WARMUP,
           "repeats": REPEATS, "worlds": {}}
    for name, w in worlds(args.arenas):
        sim = played(w)
        rec_io, rec = sim.state_io(hdr=True, counts=False, cells=True)
        yard_io, _ = sim.state_io(hdr=False, counts=False, cells=True)
        sim.state_device(rec_io)
        put_io, keep = sim.state_put_io(rec["raw"], status=True)
        snap = sim.snapshot(args.arenas)
        ident = torch.arange(args.arenas, dtype=torch.int32, device="cuda")
        snap.save(ident)
        before = sim.digest()
        calls = {"put": lambda: sim.state_put_device(put_io), "state_device": lambda: sim.state_device(yard_io),
                 "snapshot_load": lambda: snap.load(ident)}
        order = list(calls)
        med = {k: [] for k in calls}
        for rnd in range(2):
            for k in order[rnd:] + order[:rnd]:
                med[k].append(series(calls[k], sim.synchronize))
        assert np.array_equal(sim.digest(), before) and int((keep["status"] != 0).sum()) == 0  # (what is timed is right)
        rd, wr = must_move(w.cfg)
        total = (rd + wr) * args.arenas
        put, yard = statistics.mean(med["put"]), statistics.mean(med["state_device"])
        spread = abs(med["state_device"][0] - med["state_device"][1])
        res = {"median_ms": med, "bytes_read": rd * args.arenas, "bytes_written": wr * args.arenas, "ms_at_copy_rate": total / COPY_RATE * 1e3,
               "put_over_copy_rate": put / (total / COPY_RATE * 1e3), "put_over_state_device": put / yard,
               "state_device_spread_ms": spread, "within_twice_state_device_plus_spread": bool(put <= 2 * yard + spread)}
        out["worlds"][name] = res
        snap.close(), sim.close()
        print(name, json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
