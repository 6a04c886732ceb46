#!/usr/bin/env python3
"""Generates the online `.sf_sample` fixtures: tests/golden/online_plain.sf_sample, online_quit.sf_sample and
online_samples.json.  Two three-player Battle matches on the REFERENCE's own match server (oracle/_ref/sf_match_server),
with the REFERENCE's own client (oracle/_ref/sf_ref_tick, logging on) in seat 1 and two strikeforce_amd.lockstep clients
in seats 0 and 2 — the harness of tests/test_lockstep_server.py:

    online_plain   120 iterations, nobody leaves
    online_quit    120 iterations, seat 2 sends '_' in iteration 50 (the 51st): from then on an iteration logs two lines

Every player has the same level-1 character record, so that Human::log_file / scan_file level nobody's start values up
twice (tests/test_ref_replay.py).  The two `.sf_sample` files are committed exactly as the reference client wrote them
(layout "logged" of strikeforce_amd/replay.py); online_samples.json holds, per match, what the file does not say (the
teams, the map's parameters, the pools) and the 64-bit state digest of the reference client's OWN dump after the
placement and after every iteration (the recipe of make_ref_traj.py, whose digest_of this imports).  A shadow oracle in
the reference client's seat, fed the commands the match relayed, must equal the reference client's dump at every one of
those moments: a fixture can only come from a run in which they agree.  Needs the reference checkout (oracle/_ref/).

    python tests/golden/make_online_sample.py
"""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib  # noqa: E402
import reftick  # noqa: E402
import test_lockstep_server as harness  # noqa: E402
from make_ref_traj import digest_of  # noqa: E402
from strikeforce_amd import abi, config, lockstep  # noqa: E402

# 15000 Hp / 1000 damage / 15000 stamina at level 1 in every mode: nobody dies in 120 iterations, nothing is levelled up
RECORD = [15000, 1000, 15000, 1, 1, 1, 300000, 60, 0, 0, 0, 1, 1, 1, 34] + [1] * 16 + [56]
MAP = dict(rows=28, cols=36, wall_p=0.04, portal_pairs=1)
POOLS = dict(H=12, Z=10, B=48, P=48)  # (the reference pools exits by B, `portal[B]` gameplay.hpp:51-53)
TEAMS = [1, 2, 3]
TICKS = 120
SEAT = 1  # the reference client's


def play_match(quit_at=None, record=None):
    """quit_at: (seat, iteration) of the lock-step client that leaves with '_'; record: every player's character record
    (RECORD).  Returns the log's text, the facts and the reference client's dumps by iteration (-1: the placement)."""
    record = record or RECORD
    port, password = harness._free_port(), "sesame"
    proc = harness._start_server(port, password, TEAMS)
    m, portal = config.synthetic_map(MAP["rows"], MAP["cols"], wall_p=MAP["wall_p"], portal_pairs=MAP["portal_pairs"])
    cfg0 = config.make_config(1, MAP["rows"], MAP["cols"], mode=abi.MODE_BATTLE, n_agents=3, teams=TEAMS, auto_reset=0,
                              player_tokens=record, **POOLS)
    ref = reftick.RefTick(config.Workload("match", cfg0, m, portal), record, native_caps=False)
    errors, ours, relayed, ref_dumps, info = [], {}, {}, {}, {}

    def ref_thread():
        try:
            ref.logging(True)
            tb, serial, ind, n, team = ref.join_match("127.0.0.1", port, password)
            info.update(tb=tb, serial=serial, ind=ind, n=n, team=team)
            rng = np.random.RandomState(77)
            ref_dumps[-1] = ref.dump()
            for it in range(TICKS):
                ref.step(abi.BENCH_COMMANDS[rng.randint(0, 28)])
                ref_dumps[it] = ref.dump()
                assert not ref.over, "the reference holds more entities than the pools"
            info["text"] = open(ref.logclose()).read()
        except Exception as e:  # noqa: BLE001
            errors.append(("reference client", repr(e)))

    def our_thread(k):
        try:
            c = lockstep.MatchClient("127.0.0.1", port, password, record, name="p%d" % k).connect()
            sim = oracle_lib.Oracle(c.workload(MAP["rows"], MAP["cols"], m, portal, **POOLS))
            ours[c.ind] = c
            rng = np.random.RandomState(1000 + c.ind)

            def policy(_sim, it):
                if quit_at is not None and (c.ind, it) == tuple(quit_at):
                    return "_"
                return abi.BENCH_COMMANDS[rng.randint(0, 28)]

            step0 = sim.step

            def step(cmd):
                relayed.setdefault(c.ind, []).append(bytes(cmd))
                step0(cmd)
            sim.step = step
            lockstep.play(c, sim, policy, max_iterations=TICKS)
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=ref_thread) if k == SEAT else threading.Thread(target=our_thread, args=(k,))
               for k in range(3)]
    for t in threads:
        t.start()
        time.sleep(0.4)  # connection order = player index
    for t in threads:
        t.join(timeout=180)
    ref.close()
    try:
        proc.stdin.write("done!\n")
        proc.stdin.flush()
        proc.wait(timeout=20)
    except Exception:  # noqa: BLE001
        proc.kill()
    assert not errors, errors
    assert (info["ind"], info["n"], info["team"]) == (SEAT, 3, TEAMS[SEAT])
    c0 = ours[0]
    assert (c0.tb, c0.serial) == (info["tb"], info["serial"]) and len(relayed[0]) == TICKS
    # the shadow: this repo's simulation as the reference client's process sees the match
    cfg = config.make_config(1, MAP["rows"], MAP["cols"], mode=abi.MODE_BATTLE, level=1, n_agents=3, teams=c0.teams,
                             auto_reset=0, player_tokens=record, ind=SEAT, agent_tokens=c0.records, **POOLS)
    shadow = oracle_lib.Oracle(config.Workload("shadow", cfg, m, portal))
    shadow.reset((C.c_uint64 * 1)(c0.tb), (C.c_uint64 * 1)(c0.serial))
    digests = []
    for it in range(-1, TICKS):
        if it >= 0:
            shadow.step(np.frombuffer(relayed[0][it], dtype=np.uint8))
        od = shadow.dump(0)
        d = reftick.first_difference(ref_dumps[it], reftick.arrays_of(od))
        assert d is None, "iteration %d: %s" % (it, d)
        assert not od.hdr.done, "the game ended at iteration %d" % it
        dg = digest_of(ref_dumps[it], od, cfg)
        assert dg == int(shadow.digest()[0])
        digests.append("%016x" % dg)
    facts = {"tb": info["tb"], "serial": info["serial"], "players": 3, "ind": SEAT, "teams": list(c0.teams),
             "iterations": TICKS, "quit": list(quit_at) if quit_at else None, "map": MAP, "pools": POOLS,
             "digests": digests}
    return info["text"], facts, ref_dumps


if __name__ == "__main__":
    if not reftick.available() or not os.path.exists(harness.SERVER):
        raise SystemExit("oracle/_ref/ is not built: needs the reference checkout (python __graft_entry__.py)")
    data = {"_generator": "tests/golden/make_online_sample.py: the .sf_sample files are what oracle/_ref/sf_ref_tick (the "
                          "reference's client, head-less) logged in seat 1 of a match on oracle/_ref/sf_match_server; the "
                          "digests are of that client's own state dumps", "matches": {}}
    for name, quit_at in (("online_plain", None), ("online_quit", (2, 50))):
        text, facts, _ = play_match(quit_at)
        facts["file"] = name + ".sf_sample"
        facts["tokens"] = len(text.split())
        with open(os.path.join(HERE, facts["file"]), "w") as f:
            f.write(text)
        data["matches"][name] = facts
        print(name, facts["tokens"], "tokens,", len(facts["digests"]), "digests")
    with open(os.path.join(HERE, "online_samples.json"), "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote online_samples.json")
