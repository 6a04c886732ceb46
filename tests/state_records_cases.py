"""The small worlds of the sf_state_device tests, each played to the step where it is used, and what their states must hold
between them (features(); tests/test_state_records_cases.py asserts it from the oracle alone).  The shapes are the smallest
at which the kernel's traversal can go wrong: 1 / 3 / 65 arenas, human pools of 8 and 22, zombie pools of 24 / 64 / 200 (the
large-pool path), bullet pools of 64 and 128, exit pools of 16 and 109, maps of 63 cells, 64 x 64 and 128 x 128 (flag plane in
HBM).  Test helper only."""
import types

import numpy as np

from oracle_lib import Oracle
from strikeforce_amd import abi, config

QUIT, NOP = ord("_"), ord("+")


def _tiny(A):  # 63 cells: not a multiple of 4, 16 or 64; Timer games of 20 steps under auto_reset: restarted arenas
    cfg = config.make_config(A, 9, 7, H=8, Z=24, B=64, P=16, mode=abi.MODE_TIMER, auto_reset=1, timer_frames=40)
    return config.Workload("st-tiny", cfg, *config.synthetic_map(9, 7, wall_p=0.0))


def _mid(A):  # configs[2]'s map with the pools at a full 64-slot batch and at two of them; a Battle of eight with guns
    cfg = config.make_config(A, 64, 64, H=8, Z=64, B=128, P=16, mode=abi.MODE_BATTLE, n_agents=8,
                             teams=[1 + (i % 2) for i in range(8)], auto_reset=1)
    return config.Workload("st-mid", cfg, *config.synthetic_map(64, 64, wall_p=0.03))


def _battle(A):  # 22 human slots, 109 exits (more than 64: the large-pool step kernels), games that end and stand still
    cfg = config.make_config(A, 64, 64, H=22, Z=24, B=64, P=109, mode=abi.MODE_BATTLE, n_agents=8,
                             teams=[1 + (i % 3) for i in range(8)], auto_reset=0)
    return config.Workload("st-battle", cfg, *config.synthetic_map(64, 64, wall_p=0.03, portal_pairs=2))


def _large(A):  # three floors, 200 zombie slots: three whole batches and a tail of 8
    cfg = config.make_config(A, 20, 30, floors=3, H=22, Z=200, B=128, P=109, mode=abi.MODE_SQUAD, n_agents=3, level=10, auto_reset=0)
    return config.Workload("st-large", cfg, *config.three_floor_map(20, 30))


def _hbm(A):  # configs[3]'s map (128 x 128: the flag plane stays in HBM), Squad: blocks and portals get built
    cfg = config.make_config(A, 128, 128, H=10, Z=24, B=64, P=16, mode=abi.MODE_SQUAD, auto_reset=0)
    keep = [(0, 3, 1)] + [(0, 1, i + 1) for i in range(1, 10)]
    return config.Workload("st-hbm", cfg, *config.synthetic_map(128, 128, portal_pairs=2, keep_clear=keep))


def _swarm(A):  # the large zombie pool in use: a player that outlives 3500 steps of a Timer game, 70 to 90 zombies alive
    tough = list(config.HUMAN_ENEMY_TOKENS)
    tough[0] = 100_000_000
    cfg = config.make_config(A, 20, 30, floors=3, H=8, Z=200, B=64, P=16, mode=abi.MODE_TIMER, level=10, auto_reset=0, player_tokens=tough)
    return config.Workload("st-swarm", cfg, *config.three_floor_map(20, 30))


def _rows(w, steps, seed):
    return config.bench_commands(w.cfg.arenas, w.cfg.n_agents, steps, seed0=seed)[0].reshape(steps, w.cfg.arenas, w.cfg.n_agents).copy()


def _battle_rows(w, steps, seed):
    rows = _rows(w, steps, seed)
    rows[5, 0, 3] = QUIT  # a commanded human that is dead while its game goes on
    rows[steps - 2, 1, :] = QUIT  # everybody quits: arena 1 is finished (done, outcome) and stands still
    return rows


def _gun_rows(w, steps, seed):
    """Everybody takes the AK_47 ('m'), then fires, turns and walks: bullets that enter one cell, one of them orphaned."""
    rows = np.frombuffer(b"xxxqewasd", dtype=np.uint8)[_rows(w, steps, seed) % 9].copy()
    rows[0] = ord("m")
    return rows


def _still_rows(w, steps, seed):
    return np.full((steps, w.cfg.arenas, w.cfg.n_agents), NOP, dtype=np.uint8)


#        name     world   arenas steps seed  rows
CASES = [("tiny", _tiny, 3, 47, 21, _rows),
         ("mid", _mid, 65, 17, 22, _gun_rows),
         ("battle", _battle, 3, 30, 23, _battle_rows),
         ("large", _large, 3, 1500, 24, _rows),
         ("swarm", _swarm, 3, 3500, 26, _still_rows),
         ("hbm", _hbm, 1, 120, 25, _rows)]
NAMES = [c[0] for c in CASES]
_cache = {}


def case(name):
    """The case's world (a fresh Workload), its command rows uint8 [steps][arenas][n_agents] and its seeds."""
    _, world, A, steps, seed, rows = CASES[NAMES.index(name)]
    w = world(A)
    tb, sr = w.seeds(base_tb=1_700_001_000 + 1000 * NAMES.index(name))
    return types.SimpleNamespace(name=name, w=w, rows=rows(w, steps, seed), tb=tb, sr=sr)


def oracle_dumps(name):
    """The oracle's dump of every arena after the case's last step, and its digests: computed once per process and shared
    (nobody writes into them)."""
    if name not in _cache:
        c = case(name)
        o = Oracle(c.w)
        try:
            o.reset(c.tb, c.sr)
            o.step_many(c.rows)
            _cache[name] = ([o.dump(a) for a in range(c.w.cfg.arenas)], o.digest())
        finally:
            o.close()
    return _cache[name]


def features(dumps, cfg):
    """Which of the states the issue lists a set of dumps of one configuration holds: {name: bool}."""
    f = dict.fromkeys(("bullet_ref1", "bullet_ref0", "bullet_negative_effect", "super_zombie", "dead_commanded_human", "unused_slot",
                       "human_upstairs", "built_block_damaged", "built_entrance_and_map_entrance", "inactive_exit_between_active",
                       "finished_arena", "restarted_arena", "zombie_extent_above_64"), False)
    for d in dumps:
        for b in d.bullets:
            if b.alive:
                f["bullet_ref1"] |= b.ref == 1
                f["bullet_ref0"] |= b.ref == 0
                f["bullet_negative_effect"] |= b.effect < 0
        f["super_zombie"] |= any(z.alive and z.super_ for z in d.zombies)
        f["dead_commanded_human"] |= any(not h.alive and h.way != 0 for h in d.humans[:cfg.n_agents])
        f["unused_slot"] |= any(not any(np.frombuffer(bytes(h), dtype=np.int32)) for h in d.humans)
        f["human_upstairs"] |= any(h.alive and h.f > 0 for h in d.humans)
        temp, pin = (d.flags & abi.CELL_TEMP) != 0, (d.flags & (abi.CELL_PIN_UP | abi.CELL_PIN_DN)) != 0
        f["built_block_damaged"] |= bool((temp & ~pin & (d.dmg > 0)).any())
        f["built_entrance_and_map_entrance"] |= bool((temp & pin & (d.pidx >= 0)).any() and (~temp & pin & (d.pidx >= 0)).any())
        act = np.array([p.active for p in d.portals])
        if act.any():
            f["inactive_exit_between_active"] |= bool((act[:np.nonzero(act)[0].max()] == 0).any())
        f["finished_arena"] |= d.hdr.done != 0 and d.hdr.outcome != 0
        f["restarted_arena"] |= cfg.auto_reset != 0 and d.hdr.episodes > 0
        alive = np.array([z.alive for z in d.zombies])
        f["zombie_extent_above_64"] |= cfg.cap_zombies > 64 and alive.any() and int(np.nonzero(alive)[0].max()) + 1 > 64
    return f
