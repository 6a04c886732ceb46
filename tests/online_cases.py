"""Shared by the online `.sf_sample` tests: the fixtures of tests/golden/make_online_sample.py (two matches the
reference's own client logged on the reference's own server), the state digest recomputed from a dump, and matches played
here on the oracle and written out as samples.  Test infrastructure only; reads nothing outside tests/golden/."""
import ctypes as C
import json
import os

import numpy as np

import oracle_lib
import reftick
from strikeforce_amd import abi, config, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FACTS = json.load(open(os.path.join(GOLDEN, "online_samples.json")))["matches"]
NAMES = ("online_plain", "online_quit")
# the record every player of the fixtures and of the matches played here has (level 1: nothing is levelled up twice)
RECORD = [15000, 1000, 15000, 1, 1, 1, 300000, 60, 0, 0, 0, 1, 1, 1, 34] + [1] * 16 + [56]


def path_of(name):
    return os.path.join(GOLDEN, FACTS[name]["file"])


def load(name):
    """(sample, facts) of one fixture match, read as the layout the reference logged it in."""
    f = FACTS[name]
    return replay.read_sample(path_of(name), layout="logged", teams=f["teams"]), f


def map_of(f):
    m = f["map"]
    return config.synthetic_map(m["rows"], m["cols"], wall_p=m["wall_p"], portal_pairs=m["portal_pairs"])


def workload(sample, f, arenas=1):
    chars, portal = map_of(f)
    return replay.workload_for(sample, f["map"]["rows"], f["map"]["cols"], chars, portal, arenas=arenas, **f["pools"])


def digest_of_dump(d, cfg, done=None, outcome=None):
    """sf_digest_from_dump (oracle/sf_oracle.c, the definition sf_state_digest shares) over an ArenaDump, with hdr.done /
    hdr.outcome replaced where given."""
    L = oracle_lib.lib()
    a = reftick.arrays_of(d)
    hdr = abi.ArenaHdr()
    for n, _ in abi.ArenaHdr._fields_:
        if n != "rng":
            setattr(hdr, n, getattr(d.hdr, n))
    for i in range(18):
        hdr.rng[i] = d.hdr.rng[i]
    if done is not None:
        hdr.done, hdr.outcome = done, outcome
    tabs = [np.ascontiguousarray(a[k], dtype=np.int32) for k in ("humans", "zombies", "bullets", "portals")]
    flags = np.ascontiguousarray(a["flags"], dtype=np.uint8)
    dmg, pidx = np.ascontiguousarray(a["dmg"], np.int32), np.ascontiguousarray(a["pidx"], np.int32)
    L.sf_digest_from_dump.restype = C.c_uint64
    L.sf_digest_from_dump.argtypes = [C.c_int] * 5 + [C.c_void_p] * 8
    return int(L.sf_digest_from_dump(cfg.cap_humans, cfg.cap_zombies, cfg.cap_bullets, cfg.cap_portals, flags.size,
                                     C.addressof(hdr), tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data,
                                     tabs[3].ctypes.data, flags.ctypes.data, dmg.ctypes.data, pidx.ctypes.data))


def lines_per_iteration(sample, players_alive):
    """The sample's tokens grouped by iteration, given for every iteration which players other than `ind` take a line."""
    out, cur = [], 0
    for alive in players_alive:
        row = [0] * sample.players
        row[sample.ind] = ord(sample.commands[cur])
        cur += 1
        for g in alive:
            row[g] = ord(sample.commands[cur])
            cur += 1
        out.append(row)
    assert cur == len(sample.commands)
    return out


# ---- matches played here, on the oracle, and written out the way the reference's logger would -------------------------
BATCH = dict(map=dict(rows=28, cols=36, wall_p=0.04, portal_pairs=1), pools=dict(H=12, Z=10, B=48, P=48), teams=[1, 2, 3],
             ind=1)


def play_and_log(tb, serial, iterations, seed, quit_at=None, ind_quits_at=None):
    """One three-player Battle match on the oracle as the client in seat `ind` sees it; every player sends random
    commands (seeded), the rival in seat quit_at[0] leaves with '_' in iteration quit_at[1], `ind` itself in iteration
    ind_quits_at.  Returns the Sample the reference's logger would have written: per iteration the command of `ind`,
    then one line for every other player alive and remote when human_action runs (gameplay.hpp:966-967,979-986)."""
    f = BATCH
    proto = replay.Sample(tb, serial, RECORD, "", name="p1", ind=f["ind"], team=f["teams"][f["ind"]], players=3,
                          names=["p0", "p1", "p2"], records=[RECORD] * 3, teams=f["teams"])
    sim = oracle_lib.Oracle(workload(proto, f))
    sim.reset((C.c_uint64 * 1)(tb), (C.c_uint64 * 1)(serial))
    rng = np.random.RandomState(seed)
    lines = []
    for it in range(iterations):
        assert not sim.done()[0], "the match ended at iteration %d" % it
        cmd = np.array([ord(abi.BENCH_COMMANDS[i]) for i in rng.randint(0, 28, size=3)], dtype=np.uint8)
        if quit_at is not None and it == quit_at[1]:
            cmd[quit_at[0]] = ord("_")
        if ind_quits_at is not None and it == ind_quits_at:
            cmd[f["ind"]] = ord("_")
        lines.append(chr(cmd[f["ind"]]))
        sim.step_begin()
        alive = sim.agent_alive()[0]
        for g in range(3):
            if g != f["ind"] and alive[g]:
                lines.append(chr(cmd[g]))
        sim.step_end(cmd)
    proto.commands = "".join(lines)
    return proto


def batch_samples(tmp_dir, n=96, seed=2024):
    """n samples of 40 ... 160 iterations, written to tmp_dir and read back (both layouts in turn).  Every sixth has a
    rival that quits, every sixth is cut in the middle of its last iteration.  Returns [(sample, kind, iterations)]."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        iters = 40 + (k * 120) // (n - 1)
        kind = {1: "quit", 4: "cut"}.get(k % 6, "plain")
        quit_at = (0 if k % 12 == 1 else 2, int(rng.randint(5, iters - 5))) if kind == "quit" else None
        s = play_and_log(1_700_000_000 + 17 * k, 123_456_789 + k, iters, seed + k, quit_at=quit_at)
        if kind == "cut":  # the last iteration holds three lines: one or two of them are lost
            s.commands = s.commands[:-(1 + (k % 12 == 4))]
        layout = "replay" if k % 2 else "logged"
        p = os.path.join(str(tmp_dir), "m%03d.sf_sample" % k)
        replay.write_sample(p, s, layout=layout)
        r = replay.read_sample(p, layout=layout, teams=BATCH["teams"])
        assert (r.tb, r.serial, r.commands, r.records, r.teams) == (s.tb, s.serial, s.commands, s.records, s.teams)
        out.append((r, kind, iters))
    return out
