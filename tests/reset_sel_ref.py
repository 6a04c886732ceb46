"""What sf_reset_arenas (strikeforce.h) must leave behind, restated over the CPU oracle.  The oracle has only a whole reset,
so the restatement holds ONE single-arena oracle per arena (arenas = 1, reseed_stride set explicitly to the batch's value,
so that the seeds of auto_reset agree) and does a masked restart as that arena's own sfo_reset.  What a whole reset clears
and a masked restart must keep is kept here in plain Python: the running `episodes` ordinal and the result latch; so is the
selection rule (mask, done_too, max_steps).  Test helper only."""
import ctypes as C
import types

import numpy as np

from oracle_lib import Oracle
from strikeforce_amd import abi


def seed_stride(cfg):
    return cfg.reseed_stride if cfg.reseed_stride > 0 else cfg.arenas


def single_arena(w):
    """A workload of one arena with w's configuration (the map buffers stay w's) and the batch's seed stride."""
    cfg = abi.Config.from_buffer_copy(w.cfg)
    cfg.arenas, cfg.reseed_stride = 1, seed_stride(w.cfg)
    return types.SimpleNamespace(name=w.name, cfg=cfg, parent=w)


def choose(mask, done, steps, done_too, max_steps):
    """The selection rule: by mask, by a finished game (done_too), by a running game that has reached max_steps."""
    done, steps = np.asarray(done) != 0, np.asarray(steps)
    sel = np.zeros(len(done), dtype=bool) if mask is None else np.asarray(mask) != 0
    if done_too:
        sel = sel | done
    if max_steps > 0:
        sel = sel | (~done & (steps >= max_steps))
    return sel


class ResetSelRef:
    """Same call surface as an oracle of `arenas` arenas, plus reset_arenas()."""

    def __init__(self, w, tb, sr):
        self.w, self.cfg = w, w.cfg
        self.A, self.stride = w.cfg.arenas, seed_stride(w.cfg)
        self.sims = [Oracle(single_arena(w)) for _ in range(self.A)]
        self.reset(tb, sr)

    def close(self):
        for s in self.sims:
            s.close()

    def reset(self, tb, sr):
        for a, s in enumerate(self.sims):
            s.reset((C.c_uint64 * 1)(int(tb[a])), (C.c_uint64 * 1)(int(sr[a])))
        self.base = np.zeros(self.A, dtype=np.int64)  # episodes counted before the arena's last masked restart
        self.latch = np.zeros((self.A, self.cfg.n_agents, 8), dtype=np.int32)
        self.restarts = np.zeros(self.A, dtype=np.int64)
        self.fresh = np.ones(self.A, dtype=bool)  # no step since the arena's last (re)start

    def _latch(self, a):
        self.latch[a] = self.sims[a].results()[0]

    def step(self, cmd):
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8).reshape(self.A, self.cfg.n_agents)
        for a, s in enumerate(self.sims):
            s.step(cmd[a])
            self.fresh[a] = False
            if s.done()[0]:
                self._latch(a)  # (auto_reset == 0: a finished game's record does not change any more)

    def hdr(self, a):
        return self.sims[a].dump(0).hdr

    def reset_arenas(self, mask=None, done_too=False, max_steps=0, tb=None, serial=None):
        """Returns bool [arenas]: the arenas restarted.  tb / serial: sequences of `arenas` entries, read for the chosen
        arenas only; both None: the arena's tb + stride, its serial kept."""
        assert (tb is None) == (serial is None)
        hdrs = [self.hdr(a) for a in range(self.A)]
        sel = choose(mask, [h.done for h in hdrs], [h.steps for h in hdrs], done_too, max_steps)
        for a in np.nonzero(sel)[0]:
            h, s = hdrs[a], self.sims[a]
            ntb = (h.tb + self.stride) % (1 << 64) if tb is None else int(tb[a])
            nsr = h.serial % (1 << 64) if tb is None else int(serial[a])
            self.base[a] += h.episodes
            self.restarts[a] += 1
            self.fresh[a] = True
            s.reset((C.c_uint64 * 1)(ntb), (C.c_uint64 * 1)(nsr))
            if s.dump(0).hdr.done:  # the new game's first loop top ended it at once: latched, as sf_reset latches it
                self._latch(a)
        return sel

    # ---- what the device is compared with ----
    def dump(self, a):
        d = self.sims[a].dump(0)
        d.hdr.episodes += int(self.base[a])
        return d

    def digest(self):
        return np.array([s.digest()[0] for s in self.sims], dtype=np.uint64)

    def done(self):
        return np.array([s.done()[0] for s in self.sims], dtype=np.uint8)

    def results(self):
        return self.latch.copy()

    def episodes(self):
        return np.array([self.dump(a).hdr.episodes for a in range(self.A)], dtype=np.int64)

    def phase_draws(self, a):
        """Draws of the arena's last step by phase; all zero until the first step of a game (the counts sf_reset leaves:
        the oracle's own whole reset keeps those of the game before, which a restarted arena must not show)."""
        return [0] * 6 if self.fresh[a] else self.sims[a].phase_draws(0)
