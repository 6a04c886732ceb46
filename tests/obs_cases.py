"""Worlds, commands and reference-side window statistics for the observation kernels' limits (k_observe modes 0-4,
k_observe_redo, k_observe_list in sf_obs_kernels.hpp).  Test helper only.

Every limit of those kernels is a count over one agent's 31 x 31 window.  The statistics here restate those counts from the
ORACLE alone (its dump() and its own observation), never from the device, so that a test can say which path a window must
have taken before it looks at what the device wrote:

  cells   non-empty cells: a flag byte, or something standing on the cell         (k_observe_list: OL_CELLS, its passes)
  own     cells that need a record of their own: a human, a live zombie or a designated bullet on it, or a flag byte that is
          not one of the eight plain classes of obs_class_of                        (OBS_REC_MAX - 8: spill; OL_REC: crowded)
  nz      non-zero floats of the observation                                        (mode 3's STAGED, the list's cap)
  q_dense values in own-record cells that are not in the host-built table           (OBS_LIST_MAX)
  q_list  values in own-record cells other than 0 and 1.0's                         (OL_POWQ)

The two queue counts are taken from the oracle's mapped outputs: x -> pow(|x| / 10, 0.2) keeps the raw values of this game
(integers and thousandths below a few million) distinct in float, so "the output is not one of the table's outputs" is
"the input is not in the table".  They are exact for windows within the record limit, where every own-record cell is built
through the queue.
"""
import math

import numpy as np

import variant_cases as vc
from strikeforce_amd import abi, config

W = abi.OBS_WINDOW
W2 = W * W
MARK = 0xFFFFFFFF
PLAIN = (0x01, 0x04, 0x08, 0x10, 0x20, 0x60, 0xA0, 0xE0)  # '#', '^', 'v', 'O', chest types 0-3: sf_obs_kernels.hpp obs_class_of
CENTRE = [(14, 15), (15, 14), (15, 15), (15, 16), (16, 15)]  # the network's pov cells, Modules.hpp:114-121


def obs_map(x):
    """Custom.hpp:157 in the oracle's arithmetic: float |x| / 10, double pow, narrowed."""
    return np.float32(math.pow(float(np.float32(abs(np.float32(x))) / np.float32(10)), 0.2))


def table_outputs(cfg):
    """Outputs of the host-built constant table (sf_host.hpp: 1.0, 0.01, 0.02 and the chest constants)."""
    ins = [1.0, 0.01, 20 / 1000.0, 10 / 1000.0] + [cfg.items.cons[i][k] / 1000.0 for i in range(4) for k in range(3)]
    return np.unique(np.array([obs_map(v) for v in ins if np.float32(v) != 0], dtype=np.float32))


ONE = obs_map(1.0)


class Stats:
    """Per (arena, agent) arrays of one sampled step."""

    def __init__(self, A, G):
        self.live = np.zeros((A, G), dtype=bool)
        for n in ("cells", "own", "nz", "q_dense", "q_list"):
            setattr(self, n, np.zeros((A, G), dtype=np.int64))

    def flat(self, name):
        return getattr(self, name).reshape(-1)


def dump_occupants(d, f, r0, c0):
    """Window cells (mask [31][31]) that the dump says are stood on: humans alive, live zombies, designated bullets; and
    the cells of humans that are not alive (a dead player stays on its cell, HF_OCC)."""
    sure, maybe = np.zeros((W, W), dtype=bool), np.zeros((W, W), dtype=bool)

    def put(m, e):
        i, j = e.r - r0, e.c - c0
        if e.f == f and 0 <= i < W and 0 <= j < W:
            m[i, j] = True
    for h in d.humans:
        put(sure if h.alive else maybe, h)
    for z in d.zombies:
        if z.alive:
            put(sure, z)
    for b in d.bullets:
        if b.alive and b.ref == 1:
            put(sure, b)
    return sure, maybe


def window_flags(d, cfg, h):
    """The flag bytes of the window around human record h ([31][31] uint8; 0 outside the map)."""
    plane = d.flags.reshape(cfg.floors, cfg.rows, cfg.cols)[h.f]
    pad = np.zeros((cfg.rows + 2 * W, cfg.cols + 2 * W), dtype=np.uint8)
    pad[W:W + cfg.rows, W:W + cfg.cols] = plane
    r0, c0 = h.r - W // 2, h.c - W // 2
    return pad[r0 + W:r0 + 2 * W, c0 + W:c0 + 2 * W], r0, c0


def window_stats(o, x=None, check=False):
    """Stats of every agent's window from oracle `o`; x: its observation, if the caller already has it.  check: also
    hold the oracle's observation against its dump (who stands where)."""
    cfg = o.cfg
    A, G = cfg.arenas, cfg.n_agents
    if x is None:
        x = o.observe()
    x = x.reshape(A, G, abi.OBS_CHANNELS, W, W)
    alive = o.agent_alive()
    tab = table_outputs(cfg)
    st = Stats(A, G)
    for a in range(A):
        d = o.dump(a)
        for g in range(G):
            if not alive[a, g]:
                assert not check or not x[a, g].any()
                continue
            h = d.humans[g]
            fl, r0, c0 = window_flags(d, cfg, h)
            xa = x[a, g]
            occ = (xa[0] != 0) | (xa[1] != 0)  # describe(): channel 0 a human or zombie, channel 1 a designated bullet
            if check:
                sure, maybe = dump_occupants(d, h.f, r0, c0)
                assert not (sure & ~occ).any() and not (occ & ~(sure | maybe)).any(), (a, g)
            own = occ | ((fl != 0) & ~np.isin(fl, PLAIN))
            v = xa[:, own]
            st.live[a, g] = True
            st.cells[a, g] = int(((fl != 0) | occ).sum())
            st.own[a, g] = int(own.sum())
            st.nz[a, g] = int(np.count_nonzero(xa))
            st.q_dense[a, g] = int(((v != 0) & ~np.isin(v, tab)).sum())
            st.q_list[a, g] = int(((v != 0) & (v != ONE)).sum())
    return st


def marked(st, lim):
    """Which windows k_observe_list must mark 0xffffffff under limits `lim` (obs_flavour.PRODUCT / SMALL)."""
    return st.live & ((st.own > lim["ol_rec"]) | (st.cells > lim["ol_cells"]))


def spilled(st, lim):
    """Which windows k_observe writes through its spill path (and marks in mode 3)."""
    return st.live & (st.own > lim["rec"])


# ---- the worlds ------------------------------------------------------------------------------------------------------

class World:
    """name; make(arenas) -> Workload; commands(arenas, steps) -> uint8 [steps][arenas][n_agents]; the run's length and the
    step counts after which it is sampled; list capacities to try."""

    def __init__(self, name, make, commands, arenas, steps, samples, caps=(2048,)):
        self.name, self.make, self._commands, self.arenas, self.steps = name, make, commands, arenas, steps
        self.samples, self.caps = sorted(set(samples)), tuple(caps)

    def workload(self):
        return self.make(self.arenas)

    def commands(self, n_agents):
        return self._commands(self.arenas, n_agents, self.steps)


def _bench(seed0=12345):
    return lambda arenas, n_agents, steps: config.bench_commands(arenas, n_agents, steps, seed0=seed0)[0]


def _variant(arenas, n_agents, steps):
    assert n_agents == vc.AGENTS
    return vc.commands(arenas, steps)


def walls_world(arenas):
    """A wall-dense 64 x 64 map: two cells of three are '#', so windows hold 550..700 non-empty cells."""
    m, p = config.synthetic_map(64, 64, wall_p=0.66, map_seed=77)
    cfg = config.make_config(arenas, 64, 64, H=12, Z=8, B=32, mode=abi.MODE_BATTLE, n_agents=8, teams=list(range(1, 9)))
    return config.Workload("obs-walls", cfg, m, p)


def pool_world(Z, n=40):
    """tests/test_large_pools.py's herd world on a small map with a zombie table of Z slots."""
    def make(arenas):
        import test_large_pools
        w = test_large_pools.world(n, arenas, exits=70)
        w.cfg.cap_zombies = Z
        w.name = "obs-pools-%d" % Z
        return w
    return make


def herd_world(arenas):
    import test_large_pools
    w = test_large_pools.world(64, arenas)
    w.cfg.cap_zombies = 1024
    w.name = "obs-herd"
    return w


def _base(which):
    return lambda arenas: config.baseline_workload(which, arenas=arenas)


def _every(first, last, step):
    return list(range(first, last + 1, step))


WORLDS = {w.name: w for w in [
    # 1: OL_CELLS = 640 and the tenth compaction pass (577..640 cells); caps: the largest, and one below every count
    World("walls", walls_world, _bench(), 8, 200, _every(1, 200, 1), caps=(2048, 64)),
    # 2: variant_cases.OBS_CASES: windows beyond 64 own records (the dense spill) on 64 x 64; the HBM plane with bitmaps
    World("spill", lambda A: vc.workload(vc.BY_NAME["lds64-B256"], A), _variant, 3, 200, _every(20, 200, 1)),
    World("crowded", lambda A: vc.workload(vc.BY_NAME["hbm_bm-B256"], A), _variant, 3, 200, _every(20, 200, 10)),
    # 3: zombie tables beyond 64 slots: 1024 (read where it lies), and the staged / unstaged edge 100, 256, 257
    World("herd", herd_world, _bench(4321), 6, 4640, _every(4600, 4640, 4)),
    World("pools100", pool_world(100), _bench(4321), 6, 2400, _every(1200, 2400, 50)),
    World("pools256", pool_world(256), _bench(4321), 6, 2400, _every(1200, 2400, 50)),
    World("pools257", pool_world(257), _bench(4321), 6, 2400, _every(1200, 2400, 50)),
    # 4: the 128 x 128 HBM plane with blocks and portals; the reference's own dimensions; three floors
    World("C4", _base("C4"), _bench(), 6, 300, _every(25, 300, 25)),
    World("NATIVE", _base("NATIVE"), _bench(), 4, 600, _every(50, 600, 50)),
    World("FLOORS", _base("FLOORS"), _bench(), 6, 300, _every(25, 300, 25)),
    # the small-limits flavour's worlds (tests/obs_flavour.py)
    World("KITS", _base("KITS"), _bench(), 8, 300, _every(10, 300, 10), caps=(2048, 360)),
    World("C3", _base("C3"), _bench(), 8, 300, _every(10, 300, 10), caps=(2048, 200)),
]}
PRODUCT_WORLDS = ["walls", "spill", "crowded", "herd", "pools100", "pools256", "pools257", "C4", "NATIVE", "FLOORS"]
FLAVOUR_WORLDS = ["KITS", "C3"]


# ---- the delta calls' schedule -------------------------------------------------------------------------------------------

def delta_plan(s):
    """What the run does with its two persistent buffers before step s (0-based): (buffer, what).  Periods of 12 steps:
    five calls on buffer 0, five on buffer 1 (the first one a call "with another pointer": writes everything), then a
    plain call on the tracked buffer 1 with the caller scribbling on it and a delta call on it (writes everything), one
    more call on it; then back to buffer 0, which the caller has scribbled on meanwhile."""
    q = s % 12
    if q < 5:
        return 0, ("switch" if q == 0 else "delta")
    if q < 10:
        return 1, ("switch" if q == 5 else "delta")
    if q == 10:
        return 1, "plain-then-delta"
    return 1, "delta"


def delta_is_incremental(s):
    """Whether the delta call before step s runs as mode 2 (differences only)."""
    return delta_plan(s)[1] == "delta"


def run_oracle(world):
    """The world's run on the oracle alone: yields (steps done, oracle) at every sampled step."""
    from oracle_lib import Oracle
    w = world.workload()
    o = Oracle(w)
    o.reset(*w.seeds())
    cmds = world.commands(w.cfg.n_agents)
    done = 0
    for s in world.samples:
        if s > done:
            o.step_many(cmds[done:s])
            done = s
        yield s, o
