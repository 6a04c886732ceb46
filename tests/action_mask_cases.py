"""The small worlds of the sf_action_mask tests: maps of at most 16 x 16 cells, one to three floors, at most a few dozen steps,
each scripted so that a commanded human meets one of obey()'s guards (gameplay.hpp:695-821) in the last few steps.  What they
reach is asserted from the oracle and the truth alone by tests/test_action_mask_cases.py; the GPU test plays the same cases on
the device.  Also here: pack(), which writes the oracle's dumps as the state file of tests/action_mask/mask_main.cpp, and
truth(), which runs that program (built once per process).  Test helper only."""
import os
import subprocess
import tempfile
import types

import numpy as np

import state_records_ref as ref
from oracle_lib import Oracle
from strikeforce_amd import abi, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "action_mask", "mask_main.cpp")
BASE = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
COMMANDS = "+qe3uzxawsdfghjkl;'cvbnm,./[]_"  # SF_COMMANDS
HF_ALIVE, HF_CTRL, HF_OCC, HF_AGP_SH = 1 << 11, 1 << 15, 1 << 22, 23  # csrc/sf_types.hpp
SC_ZWN, SC_PWN = 18, 19
_programs, _dir = {}, []


def program(build="plain"):
    """The stand-alone program, built once per process (plain, or with the address and undefined-behaviour sanitizers)."""
    if build not in _programs:
        if not _dir:
            _dir.append(tempfile.mkdtemp(prefix="sf_mask_main_"))
        exe = os.path.join(_dir[0], "mask_main_" + build)
        subprocess.check_call([os.environ.get("CXX", "g++")] + BASE + BUILDS[build] + ["-o", exe, SRC])
        _programs[build] = exe
    return _programs[build]


def cells_pad_of(cells):
    return (cells + 15) & ~15  # Params::cells_pad


def pack_arena(d, cfg, map_pidx):
    """One arena's packed state from its dump, with the bits of HW_FLAGS and the scalar words no record shows as the device
    keeps them: HF_CTRL on a living commanded human and on `ind`'s corpse, HF_OCC on whoever its cell designates, the agent
    record's number, no leftovers in dead bullet slots (a cell's designated bullet is found by BA_REF alone), and the words in
    use of the large pools."""
    arr = ref.arena_arrays(d)
    e = ref.encode(arr, map_pidx)
    for i, h in enumerate(d.humans):
        made = h.way != 0
        agent = i < cfg.n_agents and (h.profile == 0 or cfg.mode == abi.MODE_SQUAD)
        mine = i == cfg.ind and made
        fl = int(e["hum"][1, i])
        if (h.alive and agent) or mine:
            fl |= HF_CTRL
        if h.alive or mine:
            fl |= HF_OCC
        if cfg.n_agent_profiles > 0 and agent and h.profile == 0:
            fl |= i << HF_AGP_SH
        e["hum"][1, i] = fl
    for i, b in enumerate(d.bullets):
        if not b.alive:
            e["bul"][:, i] = 0
    e["scal"][SC_ZWN] = (int(arr["counts"][5]) + 63) // 64
    e["scal"][SC_PWN] = (int(arr["counts"][7]) + 63) // 64
    return e


def pack(dumps, w):
    """The state file of mask_main for the arenas `dumps` of workload w."""
    map_pidx = [int(w.cfg.map_portal[i]) for i in range(w.cells)]
    return pack_encoded([pack_arena(d, w.cfg, map_pidx) for d in dumps], w)


def pack_encoded(enc, w):
    """The state file from packed arenas (pack_arena()'s dicts)."""
    cfg = w.cfg
    A, cells, pad = len(enc), w.cells, cells_pad_of(w.cells)
    soa = lambda key: np.stack([e[key] for e in enc], axis=1)  # [field][arena][slot]
    flags = np.full((A, pad), 0xEE, dtype=np.uint8)  # (the pad behind an arena's cells is never looked at)
    for a, e in enumerate(enc):
        flags[a, :cells] = e["flags"]
    hdr = np.array([A, cfg.cap_humans, cfg.cap_zombies, cfg.cap_bullets, cfg.cap_portals, cfg.floors, cfg.rows, cfg.cols, pad,
                    cfg.n_agents, cfg.mode, cfg.ind, cfg.level, cfg.n_agent_profiles, 0, 0], dtype=np.int32)
    parts = [hdr.tobytes(), bytes(cfg.player), bytes(cfg.npc), bytes(cfg.items), bytes(cfg.agent_profile)]
    parts += [np.ascontiguousarray(x).tobytes() for x in
              (soa("hum"), soa("zom"), soa("bul"), np.stack([e["por"] for e in enc]), np.stack([e["rng"] for e in enc]),
               np.stack([e["scal"] for e in enc]), flags, np.stack([e["aux_dmg"] for e in enc]),
               np.stack([e["aux_pidx"] for e in enc]))]
    return b"".join(parts)


def run_program(state_bytes, A, n_agents, build="plain", timeout=600):
    """mask_main on a state file -> (return code, stdout, mask uint32 [A][n_agents], truth uint32 [A][n_agents])."""
    with tempfile.TemporaryDirectory(prefix="sf_mask_") as d:
        state, out = os.path.join(d, "state.bin"), os.path.join(d, "out.bin")
        with open(state, "wb") as f:
            f.write(state_bytes)
        r = subprocess.run([program(build), state, out], capture_output=True, text=True, timeout=timeout)
        words = np.fromfile(out, dtype=np.uint32) if os.path.exists(out) else np.zeros(0, dtype=np.uint32)
    if words.size != 2 * A * n_agents:
        return r.returncode, r.stdout + r.stderr, None, None
    return r.returncode, r.stdout + r.stderr, words[:A * n_agents].reshape(A, n_agents), words[A * n_agents:].reshape(A, n_agents)


def truth(dumps, w, build="plain"):
    """The truth (and the CPU body's mask, which must equal it) of the arenas `dumps`: uint32 [A][n_agents]."""
    rc, text, mask, tr = run_program(pack(dumps, w), len(dumps), w.cfg.n_agents, build)
    assert rc == 0 and "mask_main ok" in text, text[-4000:]
    assert np.array_equal(mask, tr)
    return tr


# ---- the worlds ---------------------------------------------------------------------------------------------------------
def _world(name, text, floors=1, portal=None, **kw):
    """A hand-drawn map: one string per row, the floors one after the other; portal: {(f, r, c): exit number}."""
    lines = text.split()
    rows, cols = len(lines) // floors, len(lines[0])
    assert all(len(l) == cols for l in lines) and rows * floors == len(lines) and rows <= 16 and cols <= 16
    pidx = [-1] * (floors * rows * cols)
    for (f, r, c), k in (portal or {}).items():
        pidx[(f * rows + r) * cols + c] = k
    mk = lambda A: config.Workload(name, config.make_config(A, rows, cols, floors=floors, **kw), "".join(lines).encode("ascii"), pidx)
    return mk


WEAK = list(config.HUMAN_ENEMY_TOKENS)
WEAK[2] = 60  # def_stamina: two shots of weapon 0 (25 each) and the third is refused
FRAIL = list(config.HUMAN_ENEMY_TOKENS)
FRAIL[0] = 0  # def_hp 0: alive with Hp 0 from the reset to the first hit_human

PLAIN = " ".join(["." * 16] * 16)                                        # no border: the map's edge itself
FIELD = " ".join(["#" * 16] + ["#" + "." * 14 + "#"] * 14 + ["#" * 16])   # wide enough that the spawns rarely fall on the script's cells
ROOM = "###### #....# #....# #....# #....# ######"
OUT = "######## #......# #...O..# #......# ########"
SQUAD = "############ #..........# #..........# #..........# #..........# ############"
TINY = "##### #...# #...# #...# #####"
PEN = "####### #.....# #.....# #.....# #.....# #######"
YARD = "######### #.......# #.......# #.......# #.......# #.......# #########"
TOWER = ("##^v## #....# #...O# #....# ###### " * 3).strip()
TOWER_PORTAL = {(f, 0, 2): (f + 1) % 3 for f in range(3)}
TOWER_PORTAL.update({(f, 0, 3): (f - 1) % 3 for f in range(3)})

#        name        world                                                                    scripts (one per arena; per agent in Battle)   tail
CASES = [
    # the map's edge on every side: row 0 facing off the map with a gun in hand, row N - 1, column 0, column M - 1
    ("edge", _world("am-edge", PLAIN, Z=8, B=16, P=4), ["cwqq", "c" + "s" * 14, "cae", "c" + "d" * 14 + "q"], 2),
    # a plain wall ahead: 'x' charges stamina and the bullet stays in; then the stamina runs out.  Arena 1: a throwable thrown
    # and a consumable used up
    ("wall", _world("am-wall", FIELD, Z=8, B=16, P=4, player_tokens=WEAK), ["cexx++", "kxfu++"], 5),
    # a block built ahead (a bullet may enter, a step may not), an exit placed (bare 'O', portal pending), its entrance placed
    ("build", _world("am-build", FIELD, Z=8, B=16, P=4), ["ds[q]q]q+"], 8),
    # the eight blocks used up
    ("blocks", _world("am-blocks", FIELD, Z=8, B=16, P=4), ["[d" * 8 + "+"], 3),
    # the bullet pool dry: cap_bullets 1 and an AK-47 round in flight
    ("dry", _world("am-dry", FIELD, Z=8, B=1, P=4), ["qmx++"], 3),
    # the exit pool full: one slot, taken by the map's own exit
    ("exits", _world("am-exits", OUT, Z=8, B=16, P=1), ["d+"], 2),
    # Squad: the team-mates (NPC humans) stand in the row above and fire along it (bullets on the cells beside the player)
    ("squad", _world("am-squad", SQUAD, H=10, Z=8, B=16, P=4, mode=abi.MODE_SQUAD), ["ww" + "+" * 8, "w" + "+" * 9, "wwd" + "+" * 7], 8),
    # Squad with two commanded humans: the player fires an AK-47 round along row 3, which lies on the cell south of the other
    # one when the step is stored (a bullet on the cell)
    ("cross", _world("am-cross", SQUAD, H=10, Z=8, B=16, P=4, mode=abi.MODE_SQUAD, n_agents=2), [["qmx", "sd+"]], 2),
    # Battle with 2 agents on nine free cells
    ("battle2", _world("am-battle2", TINY, H=4, Z=8, B=16, P=4, mode=abi.MODE_BATTLE, n_agents=2, teams=[1, 2]),
     [["zq+", "+ez"]] * 3, 3),
    # Battle with 16 agents on twenty free cells: every weapon, consumable and throwable selected by somebody; one quits
    ("battle16", _world("am-battle16", PEN, H=16, Z=8, B=64, P=4, mode=abi.MODE_BATTLE, n_agents=16, teams=[1 + i % 2 for i in range(16)]),
     [[c + "+" + ("_" if i == 3 else "x" if i % 3 == 0 else "+") + "+" for i, c in enumerate("cvbnm,./fghjkl;'")]], 4),
    # three floors: through '^' to floor 1 and on to floor 2; 'v' beside it
    ("floors", _world("am-floors", TOWER, floors=3, portal=TOWER_PORTAL, Z=8, B=16, P=4), ["dwwaaw++"], 8),
    # the large pools: 65 zombie slots and 65 exits, the words partly in use
    ("large", _world("am-large", OUT, Z=65, B=16, P=65), ["d]q]+", "s]+++"], 4),
    # alive with Hp 0: '_' changes nothing
    ("frail", _world("am-frail", ROOM, Z=8, B=16, P=4, player_tokens=FRAIL), [""], 1),
    # a Timer game of random commands among zombies, chests and bullets
    ("mix", _world("am-mix", YARD, H=8, Z=24, B=64, P=4, mode=abi.MODE_TIMER, level=5), ("bots", 3, 40), 10),
]
NAMES = [c[0] for c in CASES]


def _plane(A):  # 128 x 128: the flag plane stays in HBM; Squad with two commanded humans; 256 bullet slots; 65 exits (large pools)
    cfg = config.make_config(A, 128, 128, H=10, Z=24, B=256, P=65, mode=abi.MODE_SQUAD, n_agents=2, auto_reset=0)
    keep = [(0, 3, 1)] + [(0, 1, i + 1) for i in range(1, 10)]
    return config.Workload("am-plane", cfg, *config.synthetic_map(128, 128, portal_pairs=2, keep_clear=keep))


# the shapes at which the kernel's traversal can go wrong, played by the random-action agent (the GPU test's own; the CPU
# tests do not walk them): 65 arenas with one human slot and every register pool full-width; 16 agents among 64 human slots
# with 65 zombie and 65 bullet slots; the HBM plane
SHAPES = [
    ("wide65", _world("am-wide65", YARD, H=1, Z=64, B=64, P=64), ("bench", 65, 6), 2),
    ("pools", _world("am-pools", PEN, H=64, Z=65, B=65, P=64, mode=abi.MODE_BATTLE, n_agents=16, teams=[1 + i % 3 for i in range(16)]),
     ("bench", 3, 5), 2),
    ("plane", _plane, ("bench", 1, 6), 2),
]
SHAPE_NAMES = [c[0] for c in SHAPES]
_cache = {}


def case(name):
    """The case's world (a fresh Workload), its command rows uint8 [steps][arenas][n_agents], its seeds, and `tail`: the mask
    is taken after each of the last `tail` states (the state after the reset counts as one)."""
    every = CASES + SHAPES
    _, world, scripts, tail = every[[c[0] for c in every].index(name)]
    if isinstance(scripts, tuple):  # random commands: the bots' nine actions, or the random-action agent's 28
        kind, A, steps = scripts
        w = world(A)
        rows = config.bench_commands(A, w.cfg.n_agents, steps, seed0=77)[0]
        if kind == "bots":
            rows = np.frombuffer(b"+xzqeawsd", dtype=np.uint8)[rows % 9]
        rows = rows.copy()
    else:
        w = world(len(scripts))
        n = w.cfg.n_agents
        per = [s if isinstance(s, list) else [s] for s in scripts]
        assert all(len(s) == n for s in per)
        steps = max(len(x) for s in per for x in s)
        rows = np.full((steps, len(per), n), ord("+"), dtype=np.uint8)
        for a, s in enumerate(per):
            for g, x in enumerate(s):
                rows[:len(x), a, g] = np.frombuffer(x.encode("ascii"), dtype=np.uint8)
    tb, sr = w.seeds(base_tb=1_700_002_000 + 1000 * [c[0] for c in every].index(name))
    return types.SimpleNamespace(name=name, w=w, rows=rows, tb=tb, sr=sr, tail=tail)


def moments(c):
    """The numbers of steps played at the moments the mask is taken: the last `tail` of 0 .. steps."""
    steps = len(c.rows)
    return list(range(max(0, steps + 1 - c.tail), steps + 1))


def oracle_moments(name):
    """[(steps played, the oracle's dump of every arena, the truth uint32 [A][n_agents])] of the case's moments: computed once
    per process and shared (nobody writes into them)."""
    if name not in _cache:
        c = case(name)
        o = Oracle(c.w)
        out = []
        try:
            o.reset(c.tb, c.sr)
            for k in range(len(c.rows) + 1):
                if k:
                    o.step(c.rows[k - 1])
                if k in moments(c):
                    dumps = [o.dump(a) for a in range(c.w.cfg.arenas)]
                    out.append((k, dumps, truth(dumps, c.w)))
        finally:
            o.close()
        _cache[name] = out
    return _cache[name]


def features(dumps, cfg):
    """Which of the guards' situations a set of dumps of one configuration holds for some present commanded human: {name:
    bool}, from the records alone."""
    names = ("edge", "wall", "built_block", "zombie", "commanded_human", "npc_human", "chest", "entrance", "bare_exit", "bullet",
             "pool_dry", "exit_pool_full", "blocks_zero", "portal_pending", "stamina_short", "item_used_up", "selection",
             "dead_agent", "upstairs", "floor2")
    f = dict.fromkeys(names, False)
    N, M = cfg.rows, cfg.cols
    for d in dumps:
        humans = {(h.f, h.r, h.c): i for i, h in enumerate(d.humans) if h.alive}
        zombies = {(z.f, z.r, z.c) for z in d.zombies if z.alive}
        bullets = {(b.f, b.r, b.c) for b in d.bullets if b.alive and b.ref}
        dry = all(b.alive for b in d.bullets)
        full = all(p.active for p in d.portals)
        for g in range(cfg.n_agents):
            h = d.humans[g]
            if not h.alive or (h.profile != 0 and cfg.mode != abi.MODE_SQUAD):
                f["dead_agent"] = True
                continue
            f["pool_dry"] |= dry
            f["exit_pool_full"] |= full and h.portals > 0 and h.portal_ind < 0
            f["blocks_zero"] |= h.blocks == 0
            f["portal_pending"] |= h.portal_ind >= 0
            f["item_used_up"] |= min(list(h.cons) + list(h.throw_cnt)) == 0
            f["selection"] |= h.vec >= 0
            f["stamina_short"] |= h.vec == 2 and h.stamina + cfg.items.weapon[h.ind][0] < 0
            f["upstairs"] |= h.f > 0
            f["floor2"] |= h.f == 2
            for dr, dc in ((1, 0), (0, 1), (-1, 0), (0, -1)):
                r, c = h.r + dr, h.c + dc
                if not (0 <= r < N and 0 <= c < M):
                    f["edge"] = True
                    continue
                fl = int(d.flags[(h.f * N + r) * M + c])
                q = (h.f, r, c)
                f["wall"] |= bool(fl & abi.CELL_WALL) and not fl & abi.CELL_TEMP
                f["built_block"] |= bool(fl & abi.CELL_WALL) and bool(fl & abi.CELL_TEMP)
                if fl & abi.CELL_WALL:
                    continue
                if q in humans:
                    f["commanded_human" if humans[q] < cfg.n_agents else "npc_human"] = True
                elif q in zombies:
                    f["zombie"] = True
                elif fl & (abi.CELL_PIN_UP | abi.CELL_PIN_DN):
                    f["entrance"] = True
                elif q in bullets:
                    f["bullet"] = True
                elif fl & abi.CELL_CHEST:
                    f["chest"] = True
                elif fl & abi.CELL_POUT:
                    f["bare_exit"] = True
    return f
