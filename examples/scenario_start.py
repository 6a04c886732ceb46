"""Start every arena from a situation you designed, on the device.

    python examples/scenario_start.py [--arenas N] [--steps K]        (defaults 4096, 400)

The reference can set a world up in one way only: replaying a logged game from tick 0 (gameplay.hpp:968-986).  Here the
records of arena 0 after a reset are read where the state lives, edited with torch, and written into all arenas:

    rec = sim.state_records(arena_ids=[0], cells=True)["raw"]         # one row of canonical records, one launch
    ... zombies moved next to the player, Hp set, a distinct tb per arena ...
    sim.put_state(rows, row_of_arena)                                 # the check and the write, three launches

The scenario: BASELINE configs[2] (64 x 64, Timer), the player with a fifth of its Hp and six zombies standing around it.
Every arena gets a time base of its own, so the games differ from the first draw on.  Then K steps of a fixed command
cycle and the outcome distribution, read once at the end.  Nothing goes through the host in between."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import abi, config, env

OUTCOMES = ("running", "died", "won", "time lost", "time won", "quit", "sample end")


def run(arenas, steps):
    w = config.baseline_workload("C3", arenas=arenas, auto_reset=0)
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    cfg = w.cfg
    one = sim.state_records(arena_ids=[0], cells=True)
    raw = {n: one["raw"][n].clone() for n in ("hdr", "humans", "zombies", "bullets", "portals", "cell_flags", "cell_dmg", "cell_portal")}
    v = env.decode_state(hdr=raw["hdr"], humans=raw["humans"], zombies=raw["zombies"])
    me = v["humans"]
    me["hp"][0, 0] //= 5
    f, r, c = int(me["f"][0, 0]), int(me["r"][0, 0]), int(me["c"][0, 0])  # (a scalar read once, before the loop)
    walls = (raw["cell_flags"][0].view(cfg.floors, cfg.rows, cfg.cols) & abi.CELL_WALL) != 0
    ring = [(dr, dc) for dr in (-2, 0, 2) for dc in (-2, 0, 2) if (dr or dc) and 0 <= r + dr < cfg.rows and 0 <= c + dc < cfg.cols
            and not bool(walls[f, r + dr, c + dc])][:6]
    z = v["zombies"]
    for name in ("alive", "f", "r", "c", "hp", "mindamage", "super_"):
        z[name][0, :] = 0
    for i, (dr, dc) in enumerate(ring):
        z["alive"][0, i], z["f"][0, i], z["r"][0, i], z["c"][0, i] = 1, f, r + dr, c + dc
        z["hp"][0, i], z["mindamage"][0, i] = 300, 40
    # one header row per arena: a time base of its own; every arena takes the one row of tables and cells
    hdr = raw["hdr"].repeat(arenas, 1)
    h = env.decode_state(hdr=hdr)["hdr"]
    h["tb"] += torch.arange(arenas, dtype=torch.int64, device=hdr.device) * 7919
    sim.put_state({"hdr": hdr})  # rows == arenas: arena a takes header a
    tables = {n: t for n, t in raw.items() if n != "hdr"}
    status2 = sim.put_state(tables, torch.zeros(arenas, dtype=torch.int32, device=hdr.device))  # everybody forks row 0
    cycle = torch.tensor(list(b"xdxsxaxw"), dtype=torch.uint8, device=hdr.device)
    cmds = cycle[torch.arange(steps, device=hdr.device) % len(cycle)][:, None].repeat(1, arenas * cfg.n_agents).contiguous()
    sim.step_device(cmds.data_ptr(), steps)
    end = sim.state_records(humans=1, zombies=0, bullets=0, portals=0)
    outcome = torch.bincount(end["hdr"]["outcome"].long(), minlength=len(OUTCOMES)).cpu().tolist()
    written = int((status2 == 0).sum())  # (the status tensor is the batch's own: this is the second put's)
    print("written %d of %d arenas, %d zombies placed around (%d, %d, %d)" % (written, arenas, len(ring), f, r, c))
    print("outcomes after %d steps: %s" % (steps, ", ".join("%s %d" % (n, k) for n, k in zip(OUTCOMES, outcome) if k)))
    print("kills per arena: mean %.2f" % float(end["hdr"]["kills"].float().mean()))
    counts = sim.put_status()
    sim.close()
    return counts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    a = ap.parse_args()
    run(a.arenas, a.steps)
