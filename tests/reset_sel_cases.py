"""The worlds the sf_reset_arenas tests run (tests/test_reset_sel_emu.py on the wave emulator, tests/test_gpu_reset_sel.py on
the device): one per built instance family of k_reset_sel, and one per game mode.  Test helper only.

  lds-nb1   configs[2] (Timer, 64 x 64, 8 humans)                          <1,0,1,0>
  lds-nb2   variant_cases lds-B128 (Battle, 16 agents)                     <2,0,1,0>
  lds-nb4   variant_cases lds-B256                                         <4,0,1,0>
  hbm-bm    configs[3] (Squad, 128 x 128: plane in HBM, bitmaps in LDS)    <1,1,1,0>
  hbm       Solo on 129 x 128 (16 512 cells: plane in HBM, no bitmaps)     <1,1,0,0>
  zl        the large-pool world below                                     <4,0,1,1>
  solo      configs[1];  kits: Battle with agent_profile[];  b8: Battle of 8 agents (n_agents 8)

The large-pool world: a Battle match of 16 players on an open 48 x 64 map that has 60 exits of its own, pools of 128
zombies and 128 exits, and as many human slots as players, so that no NPC human spawns.  The players carry 13 portals each
(every level at 10) and ten million hit points, and do little but lay portals (']') and turn: the exits they lay go behind
the map's 60 — into the table's second 64-slot word — within 250 steps, and the zombies nobody fights pile up past slot 64
in every arena by step 1700.  large_pool_reach() reads both from an oracle."""
import numpy as np

import variant_cases as vc
from strikeforce_amd import abi, config

ZL_STEPS = 1800


def _hbm_solo(arenas, auto_reset):
    cfg = config.make_config(arenas, 129, 128, H=1, Z=16, B=32, P=4, auto_reset=auto_reset)
    m, p = config.synthetic_map(129, 128)
    return config.Workload("hbm-solo", cfg, m, p)


def _battle8(arenas, auto_reset):
    cfg = config.make_config(arenas, 40, 40, H=12, Z=12, B=64, P=8, mode=abi.MODE_BATTLE, n_agents=8,
                             teams=list(range(1, 9)), auto_reset=auto_reset)
    m, p = config.synthetic_map(40, 40, wall_p=0.05, portal_pairs=1)
    return config.Workload("b8", cfg, m, p)


def _large_pools(arenas, auto_reset):
    rows, cols = 48, 64
    chars, portal = config.synthetic_map(rows, cols, wall_p=0.0, map_seed=3)
    chars = bytearray(chars)
    n = 0
    for r in range(4, rows - 4, 4):  # 10 rows x 6 exits
        for c in range(6, cols - 4, 10):
            chars[r * cols + c] = ord("O")
            n += 1
    assert n == 60
    tough = [10_000_000, 100, 1_000_000, 10, 10, 10, 1000] + [1] * 25
    cfg = config.make_config(arenas, rows, cols, H=16, Z=128, B=64, P=128, mode=abi.MODE_BATTLE, n_agents=16,
                             teams=list(range(1, 17)), auto_reset=auto_reset, player_tokens=tough)
    return config.Workload("zl", cfg, bytes(chars), portal)


WORLDS = {
    "lds-nb1": lambda A, ar: config.baseline_workload("C3", arenas=A, auto_reset=ar),
    "lds-nb2": lambda A, ar: vc.workload(vc.BY_NAME["lds-B128"], A, auto_reset=ar),
    "lds-nb4": lambda A, ar: vc.workload(vc.BY_NAME["lds-B256"], A, auto_reset=ar),
    "hbm-bm": lambda A, ar: config.baseline_workload("C4", arenas=A, auto_reset=ar),
    "hbm": _hbm_solo,
    "zl": _large_pools,
    "solo": lambda A, ar: config.baseline_workload("C2", arenas=A, auto_reset=ar),
    "kits": lambda A, ar: config.baseline_workload("KITS", arenas=A, auto_reset=ar),
    "b8": _battle8,
}
VARIANT = {"lds-nb1": (1, 0, 1, 0), "lds-nb2": (2, 0, 1, 0), "lds-nb4": (4, 0, 1, 0), "hbm-bm": (1, 1, 1, 0),
           "hbm": (1, 1, 0, 0), "zl": (4, 0, 1, 1), "solo": (1, 0, 1, 0), "kits": (1, 0, 1, 0), "b8": (1, 0, 1, 0)}
FAMILIES = ("lds-nb1", "lds-nb2", "lds-nb4", "hbm-bm", "hbm", "zl")
MODES = ("solo", "lds-nb1", "hbm-bm", "kits")  # Solo, Timer, Squad, Battle with agent_profile[]


def workload(name, arenas, auto_reset=0):
    w = WORLDS[name](arenas, auto_reset)
    assert vc.expected_variant(w.cfg) == VARIANT[name], name
    return w


def commands(name, arenas, n_agents, steps, seed=12345):
    """[steps][arenas][n_agents] uint8: the random-action agent, except in the large-pool world (portals and turns)."""
    if name != "zl":
        return config.bench_commands(arenas, n_agents, steps, seed0=seed)[0]
    r = np.random.RandomState(seed)
    table = np.frombuffer(b"]]]qe+wasd", dtype=np.uint8)
    return table[r.randint(0, len(table), size=(steps, arenas, n_agents))]


def large_pool_reach(dump):
    """(highest zombie slot alive, highest exit slot active) of an oracle dump."""
    z = max([i for i, x in enumerate(dump.zombies) if x.alive] or [-1])
    p = max([i for i, x in enumerate(dump.portals) if x.active] or [-1])
    return z, p


SELECTIONS = ("none", "all", "first", "last", "alternating")


def selection(kind, arenas):
    m = np.zeros(arenas, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[-1] = 1
    elif kind == "alternating":
        m[::2] = 1
    return m


def assert_same_state(x, y, a, what):
    """The whole state of arena a (header with `episodes`, every slot of every pool, the cell planes): dump x against y."""
    from oracle_lib import diff_dumps
    equal = bytes(x.hdr) == bytes(y.hdr) and np.array_equal(x.flags, y.flags) and np.array_equal(x.dmg, y.dmg) and \
        np.array_equal(x.pidx, y.pidx)
    for xs, ys in ((x.humans, y.humans), (x.zombies, y.zombies), (x.bullets, y.bullets), (x.portals, y.portals)):
        equal = equal and len(xs) == len(ys) and all(bytes(p) == bytes(q) for p, q in zip(xs, ys))
    if not equal:
        d = diff_dumps(x.as_dict(), y.as_dict())
        assert d is None, "%s, arena %d: %s" % (what, a, d)


POISON = 0xDEADBEEFDEADBEEF  # seed entries of arenas that are not chosen: a read of them shows up in the result
SENTINEL = 0xA5            # d_selected before the call


def seeds_for(sel, base, arenas):
    """uint64 [arenas] x 2: tb = base + a, serial = 7 * base + a where chosen, POISON elsewhere."""
    tb = np.full(arenas, POISON, dtype=np.uint64)
    sr = np.full(arenas, POISON, dtype=np.uint64)
    for a in np.nonzero(sel)[0]:
        tb[a], sr[a] = base + a, 7 * base + a
    return tb, sr
