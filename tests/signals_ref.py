"""What sf_signals_step (strikeforce.h) must write, restated in Python over the CPU oracle: the rules of the header in the
header's order, from nothing but what an oracle shows — dump (header and human records), results (the latch), and
agent_alive.  The source is anything with the oracle's surface over `arenas` arenas: an Oracle, or one of the
restatements that add what the oracle lacks (reset_sel_ref.ResetSelRef for sf_reset_arenas, snapshot_ref.SnapshotRef for
sf_snapshot_*, ReplayRef below for a replayed stream running out).  The reward is computed in numpy float32, one rounding
per multiply and per add, as the header writes it.  SignalsRef.reach collects which rule and branch every record took, for
tests/test_signals_cases.py.  Test helper only."""
import numpy as np

from reset_sel_ref import ResetSelRef
from strikeforce_amd import abi

PRESENT, DIED, ENDED, REBASED, UNRESOLVED, IDLE = (abi.SIG_PRESENT, abi.SIG_DIED, abi.SIG_ENDED, abi.SIG_REBASED,
                                                   abi.SIG_UNRESOLVED, abi.SIG_IDLE)
SF_SAMPLE_END = 6
F32 = np.float32


def alive_of(src):
    """uint8 [arenas][n_agents]: sf_agent_alive's bits of a source."""
    if hasattr(src, "sims"):  # one single-arena oracle per arena
        return np.stack([s.agent_alive()[0] for s in src.sims])
    return src.agent_alive()


def reward_of(w, credit, flags, d, outcome):
    """The header's reward: float32, separate multiply and add, in the order written."""
    r = F32(0.0)
    if flags & (REBASED | IDLE):
        return r
    if credit:
        r = F32(w.per_step)
        for j in range(6):
            t = F32(F32(w.w[j]) * F32(d[j]))
            r = F32(r + t)
    if flags & DIED:
        r = F32(r + F32(w.died))
    if (flags & ENDED) and credit and not (flags & UNRESOLVED):
        r = F32(r + F32(w.outcome[outcome & 7]))
    return r


class SignalsRef:
    def __init__(self, src):
        self.src, self.cfg = src, src.cfg
        self.A, self.n = src.cfg.arenas, src.cfg.n_agents
        self.base = [[None] * self.n for _ in range(self.A)]
        self.counts = [0, 0]  # records with UNRESOLVED, records rebased by the detection alone
        self.reach = set()

    def status(self):
        out, self.counts = tuple(self.counts), [0, 0]
        return out

    def step(self, rebase=None, weights=None):
        """(vitals int32 [A][n][16], delta int32 [A][n][8], reward float32 [A][n]) of one call."""
        w = weights if weights is not None else abi.RewardWeights()
        A, n = self.A, self.n
        vit = np.zeros((A, n, abi.VITALS_WORDS), dtype=np.int32)
        dlt = np.zeros((A, n, abi.DELTA_WORDS), dtype=np.int32)
        rew = np.zeros((A, n), dtype=np.float32)
        alive, latch = alive_of(self.src), self.src.results()
        for a in range(A):
            dump = self.src.dump(a)
            h = dump.hdr
            arena = (int(h.tb), int(h.serial), int(h.steps), int(h.episodes), 1 if h.done else 0)
            for g in range(n):
                hu = dump.humans[g]
                present = bool(alive[a][g])
                cur = [hu.kills, int(h.teams_kills), int(h.loot), hu.damage, hu.effect, hu.hp]
                b = self.base[a][g]
                announced = rebase is not None and rebase[a][g] != 0
                flags, d, outcome, credit = (PRESENT if present else 0), [0] * 6, 0, False
                if b is not None:
                    (btb, bsr, bsteps, beps, bdone), bcur, was = b
                    nn, ds = arena[3] - beps, arena[2] - bsteps
                    detected = nn < 0 or (nn == 0 and ((arena[0], arena[1]) != (btb, bsr) or ds < 0))
                if b is None or announced or detected:  # rule 1
                    flags |= REBASED
                    if b is not None and not announced:
                        self.counts[1] += 1
                    why = "first" if b is None else "announced" if announced else "whole-reset" if nn < 0 else \
                        "seed" if (arena[0], arena[1]) != (btb, bsr) else "steps"
                    self.reach.add("rule1:" + why)
                elif nn >= 2:  # rule 2
                    flags |= ENDED | UNRESOLVED
                    outcome, credit = int(latch[a][g][7]), was
                    self.reach.add("rule2")
                elif nn == 1:  # rule 3
                    flags |= ENDED
                    outcome, credit = int(latch[a][g][7]), was
                    if was:
                        d = [int(latch[a][g][j]) - bcur[j] for j in range(6)]
                    self.reach.add("rule3:" + ("present" if was else "absent"))
                    self.reach.add("outcome:%d" % outcome)
                    if was and not hu.alive and g != self.cfg.ind:
                        self.reach.add("rule3:died-in-the-last-step")
                else:  # rule 4
                    credit = was
                    if h.done and bdone:
                        flags |= IDLE
                        self.reach.add("idle")
                    if h.done and not bdone:
                        flags |= ENDED
                        outcome = int(h.outcome)
                        self.reach.add("rule4:newly-done:%d" % outcome)
                    if was:
                        if present:
                            d = [cur[j] - bcur[j] for j in range(6)]
                            self.reach.add("rule4:present")
                        elif not hu.alive and ds == 1:
                            d = [cur[j] - bcur[j] for j in range(6)]
                            self.reach.add("rule4:corpse")
                        else:
                            d = [0, cur[1] - bcur[1], cur[2] - bcur[2], 0, 0, -bcur[5]]
                            if ds > 1:
                                flags |= UNRESOLVED
                            self.reach.add("rule4:gone:%s:%s" % ("slot-alive" if hu.alive else "slot-empty",
                                                                 "one-step" if ds == 1 else "steps"))
                        if not present:
                            flags |= DIED
                    else:
                        self.reach.add("rule4:absent")
                if flags & UNRESOLVED:
                    self.counts[0] += 1
                self.base[a][g] = (arena, cur, present)
                for bit, name in ((PRESENT, "PRESENT"), (DIED, "DIED"), (ENDED, "ENDED"), (REBASED, "REBASED"),
                                  (UNRESOLVED, "UNRESOLVED"), (IDLE, "IDLE")):
                    if flags & bit:
                        self.reach.add("flag:" + name)
                d = [((x + 2 ** 31) % 2 ** 32) - 2 ** 31 for x in d]  # int32 arithmetic wraps
                v = [flags] + ([hu.hp, hu.stamina, hu.mindamage, hu.kills, hu.damage, hu.effect, hu.f, hu.r, hu.c, hu.way,
                                hu.team] if present else [0] * 11) + [int(h.kills), int(h.teams_kills), int(h.loot), int(h.steps)]
                vit[a][g] = v
                dlt[a][g] = [flags] + d + [outcome]
                rew[a][g] = reward_of(w, credit, flags, d, outcome)
        return vit, dlt, rew


class ReplayRef(ResetSelRef):
    """sf_replay_load / sf_replay_step for worlds with one commanded human (one line per iteration) and auto_reset 0: an
    arena whose game goes on and whose stream is used up stops with done = 1, outcome = SF_SAMPLE_END and nothing else
    changed; no episode is counted and nothing is latched."""

    def __init__(self, w, tb, sr, streams):
        assert w.cfg.n_agents == 1 and w.cfg.auto_reset == 0
        self.streams = [bytes(s) for s in streams]
        ResetSelRef.__init__(self, w, tb, sr)

    def reset(self, tb, sr):
        ResetSelRef.reset(self, tb, sr)
        self.cursor = [0] * self.A
        self.stopped = [False] * self.A

    def replay_step(self):
        for a, s in enumerate(self.sims):
            if self.stopped[a] or s.dump(0).hdr.done:
                continue
            if self.cursor[a] == len(self.streams[a]):
                self.stopped[a] = True
                continue
            s.step(np.array([self.streams[a][self.cursor[a]]], dtype=np.uint8))
            self.cursor[a] += 1
            if s.done()[0]:
                self._latch(a)

    def dump(self, a):
        d = ResetSelRef.dump(self, a)
        if self.stopped[a]:
            d.hdr.done, d.hdr.outcome = 1, SF_SAMPLE_END
        return d
