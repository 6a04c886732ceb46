"""What the episode log (strikeforce.h sf_episode_log) must hold, from the oracle stepped one step at a time: an episode's
record is sfo_results of its arena read right after the step whose sfo_done was > 0, behind the header the log defines.
Test helper only."""
import numpy as np

from strikeforce_amd import env


def seed_stride(cfg):
    return cfg.reseed_stride if cfg.reseed_stride > 0 else cfg.arenas


class OracleEpisodes:
    """Wraps an oracle (or anything with its call surface): step() / step_begin() + step_end() as the oracle's, and
    .records[a] = the records of arena a's finished episodes, in order."""

    def __init__(self, sim, tb, sr):
        self.sim, self.cfg = sim, sim.cfg
        self.tb0 = [int(x) for x in tb]
        self.sr = [int(x) for x in sr]
        sim.reset(tb, sr)
        A = self.cfg.arenas
        self.records = [[] for _ in range(A)]
        self.steps = np.zeros(A, dtype=np.int64)
        self.over = np.zeros(A, dtype=bool)   # auto_reset == 0: the arena has ended its one game and stands still
        self.first = np.zeros(A, dtype=np.int64)  # episodes counted when the log came on: earlier ones are not offered

    def log_on(self):
        """sf_episode_log(depth > 0) now: only games that end from here on are offered; their numbers go on counting."""
        self.first = self.ended().astype(np.int64)
        return self.first.copy()

    def _after_step(self):
        self.steps += 1
        done = self.sim.done()
        if not done.any():
            return
        res = self.sim.results()
        stride = seed_stride(self.cfg)
        for a in np.nonzero(done)[0]:
            assert done[a] == 1  # one loop iteration ends at most one episode
            if self.over[a]:
                continue  # (auto_reset == 0: sfo_done stays 1 after the end; there is no further episode)
            ep = len(self.records[a])
            tb = (self.tb0[a] + ep * stride) % (1 << 64)
            hdr = [a, ep, tb & 0xffffffff, tb >> 32, self.sr[a] & 0xffffffff, self.sr[a] >> 32, self.steps[a],
                   int(res[a, 0, 7])]
            rec = np.concatenate([np.array(hdr, dtype=np.uint64).astype(np.uint32).view(np.int32),
                                  res[a].reshape(-1)]).astype(np.int32)
            self.records[a].append(rec)
            self.steps[a] = 0
            if not self.cfg.auto_reset:
                self.over[a] = True

    def step(self, cmd):
        self.sim.step(cmd)
        self._after_step()

    def step_split(self, cmd):
        self.sim.step_begin()
        self.sim.step_end(cmd)
        self._after_step()

    def ended(self):
        return np.array([len(r) for r in self.records])

    def ring(self, depth, upto=None):
        """The raw rings as they must be: [arenas][depth][record words], episode e in slot e & (depth - 1), -1 where empty.
        Episodes before log_on() are not in them; upto[a] (an earlier ended()) gives the rings as they were then."""
        rw = env.episode_record_words(self.cfg.n_agents)
        out = np.full((self.cfg.arenas, depth, rw), -1, dtype=np.int32)
        for a, recs in enumerate(self.records):
            n = len(recs) if upto is None else int(upto[a])
            for e in range(max(int(self.first[a]), n - depth), n):
                out[a, e & (depth - 1)] = recs[e]
        return out

    def since(self, counts, upto=None):
        """Records of arena-ascending, episode-ascending order, each arena from its episode counts[a] on (up to upto[a])."""
        rw = env.episode_record_words(self.cfg.n_agents)
        rows = [r for a, recs in enumerate(self.records)
                for r in recs[int(counts[a]):(None if upto is None else int(upto[a]))]]
        return np.array(rows, dtype=np.int32).reshape(-1, rw)


def collect_like_kernel(ring, episodes, cursors, max_records):
    """sf_episodes_device restated on the host from the raw rings: (records, counts, new cursors)."""
    A, depth, rw = ring.shape
    out, lost, pend_left = [], 0, 0
    cur = np.array(cursors, dtype=np.int64).copy()
    for a in range(A):
        pend = max(int(episodes[a]) - int(cur[a]), 0)
        kept = min(pend, depth)
        give = min(max(max_records - len(out), 0), kept)
        first = int(episodes[a]) - kept
        for e in range(first, first + give):
            out.append(ring[a, e & (depth - 1)])
        lost += pend - kept
        pend_left += kept - give
        cur[a] += (pend - kept) + give
    recs = np.array(out, dtype=np.int32).reshape(-1, rw)
    return recs, (len(out), lost, pend_left), cur
