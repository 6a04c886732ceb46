"""The continuations of the sf_state_put_device tests: for each world of tests/state_records_cases.py, command rows played
on from the state the case ends in, drawn with another bench_commands seed than the case's own.  45 steps for `tiny` (Timer
games of 20 steps under auto_reset: at least two games end per arena, so a wrong seed digit or a wrong arming of the next
episode's generator shows), 40 for the others.  Test helper only."""
import numpy as np

import state_records_cases as sc
from oracle_lib import Oracle
from strikeforce_amd import config

STEPS = {"tiny": 45}
SEED = 900  # + the case's index: no case's own seed (21 .. 26)
_cache = {}


def continuation(name):
    """uint8 [steps][arenas][n_agents]"""
    c = sc.case(name)
    steps, cfg = STEPS.get(name, 40), c.w.cfg
    rows = config.bench_commands(cfg.arenas, cfg.n_agents, steps, seed0=SEED + sc.NAMES.index(name))[0]
    return rows.reshape(steps, cfg.arenas, cfg.n_agents).copy()


def oracle_continuation(name):
    """The oracle played through the case and then the continuation: (digests uint64 [steps + 1][arenas] — before the first
    continuation step and after every one —, episodes int64 [2][arenas] before and after, done uint8 [arenas], results and the
    headers at the end).  Computed once per process and shared (nobody writes into them)."""
    if name not in _cache:
        c = sc.case(name)
        rows = continuation(name)
        A = c.w.cfg.arenas
        o = Oracle(c.w)
        try:
            o.reset(c.tb, c.sr)
            o.step_many(c.rows)
            dig, eps0 = [o.digest().copy()], [o.dump(a).hdr.episodes for a in range(A)]
            for r in rows:
                o.step(r)
                dig.append(o.digest().copy())
            eps1 = [o.dump(a).hdr.episodes for a in range(A)]
            _cache[name] = (np.array(dig, dtype=np.uint64), np.array([eps0, eps1], dtype=np.int64), np.array(o.done()).copy(),
                            np.array(o.results()).copy(), [o.dump(a).hdr for a in range(A)])
        finally:
            o.close()
    return _cache[name]
