"""What sf_snapshot_save / sf_snapshot_load (strikeforce.h) must leave behind, restated over the CPU oracle.  The oracle has
no clone, but the game is deterministic: the restatement keeps, per arena, the seed of the sf_reset its game line started
from and every command row played since, plus ONE single-arena oracle (arenas = 1, reseed_stride set explicitly to the
batch's, so that the seeds of auto_reset agree).  A slot is a copy of (seed, command history); "load slot s into arena a"
rebuilds arena a's oracle by a reset on the slot's seed and a replay of the slot's history.  What a load must keep is kept
here in plain Python: the destination's running `episodes` ordinal and its result latch.  Test helper only."""
import ctypes as C

import numpy as np

from oracle_lib import Oracle
from reset_sel_ref import seed_stride, single_arena


class SnapshotRef:
    """Same call surface as an oracle of `arenas` arenas, plus save() / load() on `slots` slots."""

    def __init__(self, w, tb, sr, slots):
        self.w, self.cfg = w, w.cfg
        self.A, self.n, self.stride = w.cfg.arenas, w.cfg.n_agents, seed_stride(w.cfg)
        self.sims = [Oracle(single_arena(w)) for _ in range(self.A)]
        self.slots = [None] * slots
        self.skipped = [0, 0]  # loads from an empty slot, indices out of range
        self.reset(tb, sr)

    def close(self):
        for s in self.sims:
            s.close()

    def _restart(self, a, seed, history):
        s = self.sims[a]
        s.reset((C.c_uint64 * 1)(seed[0]), (C.c_uint64 * 1)(seed[1]))
        if history:
            s.step_many(np.ascontiguousarray(np.stack(history), dtype=np.uint8).reshape(len(history), 1, self.n))
        self.seed[a], self.history[a] = seed, list(history)

    def reset(self, tb, sr):
        self.seed, self.history = [None] * self.A, [None] * self.A
        for a in range(self.A):
            self._restart(a, (int(tb[a]), int(sr[a])), [])
        self.base = np.zeros(self.A, dtype=np.int64)  # what the arena's shown episode count is ahead of its oracle's
        self.latch = np.zeros((self.A, self.n, 8), dtype=np.int32)

    def step(self, cmd):
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8).reshape(self.A, self.n)
        for a, s in enumerate(self.sims):
            s.step(cmd[a])
            self.history[a].append(cmd[a].copy())
            if s.done()[0]:
                self.latch[a] = s.results()[0]

    def _verdict(self, slot, loading):
        """None: the arena takes part; else why not (counted where the device counts)."""
        if slot == -1:
            return "not named"
        if not 0 <= slot < len(self.slots):
            self.skipped[1] += 1
            return "range"
        if loading and self.slots[slot] is None:
            self.skipped[0] += 1
            return "empty"
        return None

    def save(self, slot_of_arena):
        for a, slot in enumerate(int(x) for x in slot_of_arena):
            if self._verdict(slot, False) is None:
                self.slots[slot] = (self.seed[a], list(self.history[a]))

    def load(self, slot_of_arena):
        for a, slot in enumerate(int(x) for x in slot_of_arena):
            if self._verdict(slot, True) is None:
                shown = self.dump(a).hdr.episodes  # the destination's count goes on
                self._restart(a, *self.slots[slot])
                self.base[a] = shown - self.sims[a].dump(0).hdr.episodes

    def status(self):
        out, self.skipped = tuple(self.skipped), [0, 0]
        return out

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
        """Draws of the arena's last step by phase; all zero where its game line has no step yet."""
        return self.sims[a].phase_draws(0) if self.history[a] else [0] * 6
