"""Worlds, commands and launch plans for the fixed-shape step loop as it stands since the restart left the every-step path
(sf_core.hpp step_body_t under SH::FIXED: a command pointer that runs to its end, restart() on a side branch of the
loop, seeds and games ended derived in store(), frame % {30, 40, 50} as counters).  Shared by tests/test_step_fixed_lean_emu.py (wave emulator, 8 arenas) and
tests/test_gpu_step_fixed_lean.py (device, 64 arenas).  Chosen for what that change can break:

  restarts    configs[2], Timer games of 60 frames: a game ends every 30 steps, so a launch of 100 steps restarts every
              arena three times; launches of 1, 3 and 100
  every_step  configs[2], Timer games of 2 frames: every step ends a game (frame 3 at its loop top), a launch of 3 restarts
              three times
  frames      configs[2], no game ends: 120 steps (frames 1 .. 241) as 120 launches, as one, and cut on both sides of every
              multiple of 30, 40 and 50 (a launch begins at frame m P - 1, m P + 1 and m P + 3): load() must set the
              counters from any frame
  last_step   configs[2], games of 60 frames, launches that end with the step that ends the game (30, 60, 90, 120)
  no_reset    C3's shape with auto_reset off and games of 40 frames: the generic instance (auto_reset is a fixed field);
              every arena is done after 20 steps and stays as it is
  c2_restarts configs[1] (Solo: no timer): the player kills itself ('_') every 23 steps, at a step that differs from arena
              to arena, which ends the game at that step's loop top; launches of 1, 3 and 100, and launches that end with
              arena 0's suicide (steps 23 and 46)
"""
import numpy as np

import test_fixed_shape_emu as fx
from strikeforce_amd import config

C3_SHAPE, C2_SHAPE, GENERIC = fx.C3_SHAPE, fx.C2_SHAPE, -1


def _c3(timer_frames):
    def make(arenas):
        w = fx.world(arenas)
        w.cfg.timer_frames_per_level = timer_frames
        return w
    return make


def _no_reset(arenas):
    w = fx.other_world("no auto_reset", arenas)
    w.cfg.timer_frames_per_level = 40
    return w


def _c2(arenas):
    return config.baseline_workload("C2", arenas=arenas)


def _c3_commands(arenas, steps):
    return fx.commands(arenas, steps)


def _c2_commands(arenas, steps):
    cmds, _ = config.bench_commands(arenas, 1, steps)
    cmds = cmds.copy()
    s, a = np.meshgrid(np.arange(steps), np.arange(arenas), indexing="ij")
    cmds[(s + 5 * a) % 23 == 0] = ord("_")  # arena 0: steps 0, 23, 46, ..
    return cmds


def _frame_cuts(steps):
    """Launch lengths whose boundaries lie at steps m P / 2 - 1, m P / 2 and m P / 2 + 1 (frame = 1 + 2 x steps)."""
    cuts = sorted({m * h + d for h in (15, 20, 25) for m in range(1, steps // h + 1) for d in (-1, 0, 1)} | {0, steps})
    cuts = [c for c in cuts if 0 <= c <= steps]
    return [b - a for a, b in zip(cuts, cuts[1:])]


# name: (world(arenas), commands(arenas, steps), steps, instance launched, {plan name: launch lengths},
#        fewest games every arena must have ended by the end of the oracle's run)
CASES = {
    "restarts": (_c3(60), _c3_commands, 300, C3_SHAPE, {"K=1": [1] * 300, "K=3": [3] * 100, "K=100": [100] * 3}, 9),
    "every_step": (_c3(2), _c3_commands, 12, C3_SHAPE, {"K=1": [1] * 12, "K=3": [3] * 4, "K=12": [12]}, 12),
    "frames": (_c3(1300), _c3_commands, 120, C3_SHAPE, {"K=1": [1] * 120, "K=120": [120], "cuts": _frame_cuts(120)}, 0),
    "last_step": (_c3(60), _c3_commands, 120, C3_SHAPE, {"ends": [30, 30, 1, 29, 30]}, 4),
    "no_reset": (_no_reset, _c3_commands, 40, GENERIC, {"K=1": [1] * 40, "K=40": [40], "split": [19, 1, 20]}, 1),
    "c2_restarts": (_c2, _c2_commands, 120, C2_SHAPE,
                    {"K=1": [1] * 120, "K=3": [3] * 40, "K=100": [100, 20], "ends": [24, 23, 73]}, 4),
}
for _name, (_w, _c, _steps, _k, _plans, _e) in CASES.items():
    for _plan in _plans.values():
        assert sum(_plan) == _steps and min(_plan) > 0, _name


def oracle_run(name, arenas):
    """The oracle's run of a case, one step at a time: digests and sf_done [steps][arenas], and at the end the games ended
    per arena, the results and the done flags."""
    from oracle_lib import Oracle
    world, commands, steps = CASES[name][:3]
    w = world(arenas)
    o = Oracle(w)
    o.reset(*w.seeds())
    cmds = commands(arenas, steps)
    digests = np.zeros((steps, arenas), dtype=np.uint64)
    ended = np.zeros((steps, arenas), dtype=np.int64)  # sf_done behind each step: with auto_reset, a game ended in it
    for s in range(steps):
        o.step(cmds[s])
        digests[s] = o.digest()
        ended[s] = o.done()
    hdrs = [o.dump(a).hdr for a in range(arenas)]
    out = dict(digests=digests, ended=ended, auto_reset=bool(w.cfg.auto_reset), episodes=np.array([h.episodes for h in hdrs]), frames=np.array([h.frame for h in hdrs]),
               results=o.results(), done=o.done(), hdrs=hdrs, phase_draws=[o.phase_draws(a) for a in range(arenas)])
    o.close()
    return out


def done_after(run, s0, k):
    """What sf_done reports behind a launch of steps [s0, s0 + k): with auto_reset the games that ended inside the launch
    (saturating at 255), without it the arena's done flag."""
    if run["auto_reset"]:
        return np.minimum(run["ended"][s0:s0 + k].sum(axis=0), 255)
    return run["ended"][s0 + k - 1]
