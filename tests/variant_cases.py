"""One workload per built instance of the step kernels (k_reset / k_step / k_step_half <NB, HP, BM, ZL>, sf_api.hip), with
the bullet pool filled to its top word.  Test helper only.

The world: a Battle match of 16 armed agents, each its own team.  Player and NPC record human_enemy.txt with every weapon
at level 3; every agent selects weapon 4 ('m': range 100, so every shot is a bullet; weapons 0-3 'c' 'v' 'b' 'n' have
range 1 and strike the next cell without one) and then fires ('x') every step, turning ('q') now and then so that the
shots spread.  A game that ends restarts inside the launch (auto_reset) with its weapons unselected, so 'm' comes back
now and then too.  B sits at the top of its word range: the pool runs dry, every word boundary is crossed.

Agent 0 is the player: it quits ('_') every 100 steps, so every arena ends a game and starts the next one inside a launch.

Maps by flag-plane variant (sf_types.hpp), all open (border walls only): 128 x 96 (12 288 cells, the largest plane that
stays in LDS) keeps the plane in LDS; 120 x 120 (14 400 cells) puts it in HBM with the cell bitmaps in LDS; three floors of
80 x 80 (19 200 cells) put it in HBM without bitmaps.  (On 64 x 64 the shots reach the walls too soon to fill 256 slots;
that map is the crowded one the observation tests use, OBS_CASES.)"""
import numpy as np

from strikeforce_amd import abi, config

AGENTS = 16
LDS_PLANE_MAX = 12 * 1024  # sf_types.hpp
BM_CELLS_MAX = 16 * 1024   # use_bitmaps: three bitmaps of at most 6 KiB

# plane kind -> (floors, rows, cols)
MAPS = {"lds": (1, 128, 96), "hbm_bm": (1, 120, 120), "hbm": (3, 80, 80), "lds64": (1, 64, 64)}
QUIT_EVERY = 100


def _armed():
    t = list(config.HUMAN_ENEMY_TOKENS)
    t[2] = 1_000_000
    t[23:31] = [3] * 8
    return t


def _case(plane, B, Z=16, P=8):
    return {"name": "%s-B%d%s" % (plane, B, "-zl" if Z > 64 or P > 64 else ""), "plane": plane, "B": B, "Z": Z, "P": P}


# 12 word counts x plane kinds with small pools, then the large-pool (ZL) instance of each plane kind
PLANES = ("lds", "hbm_bm", "hbm")
CASES = [_case(plane, B) for B in (64, 128, 192, 256) for plane in PLANES] + \
        [_case(plane, 256, Z=100, P=100) for plane in PLANES]
# observation after the pools fill: the crowded 64 x 64 world (windows of more than 64 occupied cells) and 120 x 120
OBS_CASES = [_case("lds64", 256), _case("hbm_bm", 256)]
BY_NAME = {c["name"]: c for c in CASES + OBS_CASES}


def workload(case, arenas, auto_reset=1):
    F, N, M = MAPS[case["plane"]]
    if F == 1:
        m, p = config.synthetic_map(N, M, wall_p=0.0, map_seed=5 + N)
    else:
        m, p = config.three_floor_map(N, M, wall_p=0.0, map_seed=5)
    cfg = config.make_config(arenas, N, M, floors=F, H=24, Z=case["Z"], B=case["B"], P=case["P"], mode=abi.MODE_BATTLE,
                             n_agents=AGENTS, teams=list(range(1, AGENTS + 1)), auto_reset=auto_reset,
                             player_tokens=_armed(), npc_tokens=_armed())
    return config.Workload("variant-" + case["name"], cfg, m, p)


def commands(arenas, steps, seed=7):
    """[steps][arenas][16] uint8: 'x', with 'q' on ~5 % of agent-steps; every 16th step 'm' for all; agent 0 quits on
    every QUIT_EVERY-th step."""
    r = np.random.RandomState(seed)
    u = r.random_sample((steps, arenas, AGENTS))
    out = np.full((steps, arenas, AGENTS), ord("x"), dtype=np.uint8)
    out[u < 0.05] = ord("q")
    s = np.arange(steps)
    out[s % 16 == 0] = ord("m")
    out[s % QUIT_EVERY == QUIT_EVERY - 1, :, 0] = ord("_")
    return out


def expected_variant(cfg):
    """(NB, HP, BM, ZL) of the instance the host launches for `cfg`: sf_types.hpp hbm_plane / use_bitmaps / nb_for /
    large_pools, and sf_host.hpp Env::create (large pools: one instance, built for four bullet words)."""
    cells = cfg.floors * cfg.rows * cfg.cols
    cells_pad = (cells + 15) & ~15
    hp = cells_pad > LDS_PLANE_MAX
    bm_words = ((cells_pad + 31) // 32 + 3) & ~3
    bm = 3 * 4 * bm_words <= 6 * 1024
    zl = cfg.cap_zombies > 64 or cfg.cap_portals > 64
    nb = 4 if zl else (cfg.cap_bullets + 63) // 64
    return (nb, int(hp), int(bm), int(zl))


def variant_name(v):
    return "<%d,%d,%d,%d>" % v
