"""The cases of the episode-log tests (tests/test_episode_log_cases.py asserts what they reach from the oracle alone;
tests/test_gpu_episode_log_edges.py and tests/test_episode_log_emu.py run them on the device core).  Test helper only.

What makes them cheap: a commanded human that sends '_' has its Hp set to 0 and the game ends at the next check_end.
So `ind` sending '_' every p-th step ends a game every p steps in any mode (outcome DIED), and every OTHER commanded
human sending it at one step leaves `ind` the winner of a Battle (outcome WON).  lay_quits() lays such a schedule over any
command array; the rest of the commands stay what the world's own generator made them, so that the longer games carry
kills and damage in the words of agents other than `ind`."""
import numpy as np

import variant_cases as vc
from episode_log_ref import OracleEpisodes, collect_like_kernel
from oracle_lib import Oracle
from strikeforce_amd import config, env

QUIT = ord("_")
SF_DIED, SF_WON = 1, 2  # strikeforce.h sf_outcome


def lay_quits(cmds, periods, others_at=None, ind=0, start=0, stop=None):
    """Over cmds [steps][arenas][agents], in steps [start, stop): `ind` of arena a sends '_' on every periods[a]-th step
    counted from `start` (steps start + p - 1, start + 2p - 1, ...; 0 or None: never); at step others_at[a] (None or
    negative: never) every other commanded human of the arena sends it.  In place; returns cmds."""
    steps, A, n = cmds.shape
    stop = steps if stop is None else min(stop, steps)
    for a in range(A):
        p = periods[a] if periods is not None else 0
        if p:
            cmds[start + p - 1:stop:p, a, ind] = QUIT
        s = others_at[a] if others_at is not None else None
        if s is not None and 0 <= s < steps:
            cmds[s, a, [g for g in range(n) if g != ind]] = QUIT
    return cmds


class Case:
    """One world, its commands, and how the device is driven over them.
    depth: the log's depth; k: steps per launch (a collection follows every launch); writer: 'launch' (sf_step_device),
    'step' (sf_step) or 'split' (sf_step_begin / sf_step_end); on_at: the step in front of which the log is switched on."""

    def __init__(self, name, make_workload, cmds, depth, k, writer="launch", on_at=0, seeds=None):
        self.name, self.make_workload, self._cmds, self.depth, self.k = name, make_workload, cmds, depth, k
        self.writer, self.on_at, self._seeds = writer, on_at, seeds
        self._w = None

    def workload(self):
        if self._w is None:
            self._w = self.make_workload()
        return self._w

    def commands(self):
        if callable(self._cmds):
            self._cmds = self._cmds(self.workload().cfg)
        return self._cmds

    def seeds(self):
        w = self.workload()
        return self._seeds(w) if self._seeds else w.seeds()

    @property
    def steps(self):
        return self.commands().shape[0]

    def launches(self):
        """[(first step, steps)] from on_at on (the steps before it run with the log off, in one piece)."""
        return [(s, min(self.k, self.steps - s)) for s in range(self.on_at, self.steps, self.k)]


class OracleRun:
    """A case stepped on the oracle once: .o (OracleEpisodes), .ends[i] = episodes counted per arena behind launch i
    (.ends[-1] is in front of the first: .first), and the restatement of a collection behind every launch."""

    def __init__(self, case):
        self.case = case
        w = case.workload()
        tb, sr = case.seeds()
        self.o = o = OracleEpisodes(Oracle(w), tb, sr)
        cmds = case.commands()
        step = o.step_split if case.writer == "split" else o.step
        for s in range(case.on_at):
            step(cmds[s])
        self.first = o.log_on()
        self.ends = []
        for s0, n in case.launches():
            for s in range(s0, s0 + n):
                step(cmds[s])
            self.ends.append(o.ended().astype(np.int64))
        o.sim.close()

    def ring(self, i):
        return self.o.ring(self.case.depth, upto=self.ends[i])

    def per_launch(self):
        """[launches][arenas] games ended inside each launch."""
        return np.diff(np.array([self.first] + self.ends), axis=0)

    def collections(self, max_records=1 << 30):
        """collect_like_kernel behind every launch, the cursors carried: [(records, counts)]."""
        cur, out = self.first.copy(), []
        for i in range(len(self.ends)):
            recs, counts, cur = collect_like_kernel(self.ring(i), self.ends[i], cur, max_records)
            out.append((recs, counts))
        return out

    def records(self):
        """Every record offered (from log_on on), arena ascending, episode ascending."""
        return self.o.since(self.first)


_runs = {}


def oracle_run(case):
    if case.name not in _runs:
        _runs[case.name] = OracleRun(case)
    return _runs[case.name]


def multi_agent_reach(recs, n_agents):
    """Of records [n][words]: (records with non-zero kills or damage of an agent other than 0, records whose agents' words
    differ, set of outcomes)."""
    d = env.decode_episodes(recs, n_agents)
    res = d["results"]
    other = ((res[:, 1:, 0] != 0) | (res[:, 1:, 3] != 0)).any(axis=1)
    differ = (res != res[:, :1]).any(axis=(1, 2))
    return int(other.sum()), int(differ.sum()), set(int(x) for x in d["outcome"])


# ---- the wide worlds: 16 agents (one variant_cases world per built log instance, MAXCAP) and 6 (KITS) -----------------
WIDE_ARENAS, WIDE_DEPTH, WIDE_K = 5, 4, 40


def wide_schedule(c, k=WIDE_K):
    """Over commands of 5 arenas and launches of k = 40 steps: arena 0 ends a game every 3 steps (13 per launch: more than
    3 x depth), arena 1 every 8 (5 = depth + 1), arena 2 every 10 (4 = depth), arena 3 every 13 (3 = depth - 1); arena 4
    plays the first launch through (0), then ends one game per launch, every other one by the other agents giving up
    (WON).  Arenas 1-3 have the others give up once too, late in a game."""
    steps, arenas, n = c.shape
    assert arenas == WIDE_ARENAS
    c[c == QUIT] = ord("x")
    lay_quits(c, [3, 8, 10, 13, 0], others_at=[None, 3 * k + 6, 2 * k + 8, k + 11, None])
    for i, s0 in enumerate(range(k, steps, k)):
        if i & 1:
            c[s0 + 30, 4, 0] = QUIT
        else:
            c[s0 + 30, 4, 1:n] = QUIT
    return c


def _variant(case):
    return Case("variant-" + case["name"], lambda: vc.workload(case, WIDE_ARENAS),
                lambda cfg: wide_schedule(vc.commands(WIDE_ARENAS, 8 * WIDE_K)), WIDE_DEPTH, WIDE_K)


def _baseline(which, writer, launches, depth=WIDE_DEPTH):
    return Case("%s-%s%s" % (which, writer, "" if depth == WIDE_DEPTH else "-d%d" % depth),
                lambda: config.baseline_workload(which, arenas=WIDE_ARENAS),
                lambda cfg: wide_schedule(vc.commands(WIDE_ARENAS, launches * WIDE_K)[:, :, :cfg.n_agents].copy()),
                depth, WIDE_K, writer=writer)


# a: every log instance of k_step (variant_cases.expected_variant over these = the +log kernels of the code object)
VARIANTS = [_variant(c) for c in vc.CASES]
# b: the other two writers at width (and the launch writer on the two configurations never run with the log on)
WRITERS = [_baseline(which, writer, 12 if which == "KITS" else 4) for which in ("KITS", "MAXCAP")
           for writer in ("launch", "step", "split")]
# sf_reset empties rings of 16-agent records at depth 64 (136 x 64 words per arena: 136 passes of k_ep_late's first loop)
RESET_WIDE = _baseline("MAXCAP", "launch", 2, depth=64)
# the emulator's two: latch_results<true> under 6 and under 16 agents
EMULATED = [WRITERS[0], VARIANTS[0]]

# ---- c: arena counts, on C1 (one agent, 16-word records) ---------------------------------------------------------------
# (the oracle's cost is the games it restarts: depth 2 and launches of 13 steps keep 2050 arenas at a few seconds)
COUNT_DEPTH, COUNT_K, COUNT_LAUNCHES = 2, 13, 3
# periods whose games per launch of 13 steps are 6 (3 x depth), 1, 0, 3, 2; from launch to launch they move one arena up
# (turn -1), so that the arenas whose records the first launch's cuts leave pending, the last ones with records, end
# more games in the second launch than their rings hold: at 1, 3 and 5 arenas too a pending record is overwritten
COUNT_PERIODS, COUNT_TURN = [2, 13, 0, 4, 6], -1
# the histories: depth 4 (and 1), launches of 25 steps; games per launch 12 (3 x depth), 5, 4, 3, 1, 0, 2
HIST_DEPTH, HIST_K = 4, 25
PERIODS = [2, 5, 6, 8, 25, 0, 12]
ARENA_COUNTS = [1, 3, 5, 1023, 1025, 2050]
LARGE_ARENAS = 4099  # above 4096, no multiple of 4: five arenas per k_ep_plan thread, the last thread's run cut short
LARGE_WINDOWS = [0, 2040, 4089]  # first arenas of the runs of 10 the oracle is stepped for (thread-run boundaries: x 5)


def rotating_schedule(c, k, table=PERIODS, shift=0, turn=1):
    """In launch l (k steps) arena a ends a game every table[(a + turn * l + shift) % len(table)] steps."""
    steps, arenas, _ = c.shape
    for l, s0 in enumerate(range(0, steps, k)):
        lay_quits(c, [table[(a + turn * l + shift) % len(table)] for a in range(arenas)], start=s0, stop=s0 + k)
    return c


def c1_workload(arenas, stride=0, auto_reset=1):
    def make():
        w = config.baseline_workload("C1", arenas=arenas, auto_reset=auto_reset)
        w.cfg.reseed_stride = stride
        return w
    return make


def c1_commands(arenas, steps, k, table=PERIODS, first_arena=0, turn=1):
    c = config.bench_commands(arenas, 1, steps, seed0=12345 + first_arena)[0].copy()
    return rotating_schedule(c, k, table, shift=first_arena, turn=turn)


def count_commands(arenas, launches, first_arena=0):
    return c1_commands(arenas, COUNT_K * launches, COUNT_K, COUNT_PERIODS, first_arena=first_arena, turn=COUNT_TURN)


def _count(arenas):
    return Case("C1-A%d" % arenas, c1_workload(arenas), lambda cfg: count_commands(arenas, COUNT_LAUNCHES), COUNT_DEPTH,
                COUNT_K)


COUNTS = [_count(A) for A in ARENA_COUNTS]


def _window(first):
    """Arenas [first, first + 10) of the LARGE_ARENAS run, as an oracle of 10 arenas (reseed_stride = the run's arenas,
    the seeds and the commands those arenas have in it)."""
    return Case("C1-A%d-from-%d" % (LARGE_ARENAS, first), c1_workload(10, stride=LARGE_ARENAS),
                lambda cfg: count_commands(10, 2, first_arena=first), COUNT_DEPTH, COUNT_K,
                seeds=lambda w: w.seeds(first_arena=first))


LARGE = [_window(f) for f in LARGE_WINDOWS]


def cut(kind, episodes, cursors, depth, chunk=1):
    """max_records of a collection of the given kind, from the state in front of it (None: this state has no such cut).
    kinds: 'none' (0), 'one' (1), 'between' (the cut falls between two arenas that both have records), 'inside' (inside one
    arena's records), 'run' (inside one arena's records, the arena not the first of a k_ep_plan thread's run of `chunk`
    arenas, with records in front of it in that run), 'total', 'total-1'."""
    kept = np.minimum(np.maximum(np.asarray(episodes) - np.asarray(cursors), 0), depth)
    off = np.concatenate([[0], np.cumsum(kept)])
    total, has = int(off[-1]), np.nonzero(kept)[0]
    if kind == "none":
        return 0
    if kind == "one":
        return 1 if total > 1 else None
    if kind == "total":
        return total if total else None
    if kind == "total-1":
        return total - 1 if total > 1 else None
    if kind == "between":
        return int(off[has[len(has) // 2]]) if len(has) >= 2 else None
    if kind == "inside":
        wide = [a for a in has if kept[a] >= 2]
        return int(off[wide[len(wide) // 2]]) + 1 if wide else None
    if kind == "run":
        ok = [a for a in has if kept[a] >= 2 and a % chunk and kept[a - a % chunk:a].sum()]
        return int(off[ok[len(ok) // 2]]) + 1 if ok else None
    raise ValueError(kind)


# behind launch 0 / 1 / 2 of a COUNTS case, in this order ('all': uncut).  The first launch's cuts leave records pending:
# the second launch overwrites some of them before the next collection
CUTS = [["none", "one", "between", "inside", "run"], ["total-1", "all"], ["total", "all"]]


def plan_chunk(arenas):
    """Arenas per thread of k_ep_plan (sf_api.hip: 1024 threads, consecutive runs)."""
    return (arenas + 1023) // 1024


def collection_script(run, cuts=CUTS):
    """The collections of a COUNTS case from the oracle alone, the cursors carried from call to call:
    [(launch, kind, max_records, records, (written, lost, pending), cursors behind the call)]."""
    case = run.case
    A = case.workload().cfg.arenas
    cur, out = run.first.copy(), []
    for i, kinds in zip(range(len(run.ends)), cuts):
        ring = run.ring(i)
        for kind in kinds:
            mr = A * case.depth if kind == "all" else cut(kind, run.ends[i], cur, case.depth, plan_chunk(A))
            if mr is None:
                continue
            recs, counts, cur = collect_like_kernel(ring, run.ends[i], cur, mr)
            out.append((i, kind, mr, recs, counts, cur.copy()))
    return out

# ---- d: histories ------------------------------------------------------------------------------------------------------
HIST_ARENAS = 8
# the log switched on behind 25 steps: episode counts 12, 5, 4, 3, 1, 0, 2, 12: four of them no multiple of the depth
LATE_ON = Case("C1-late-on", c1_workload(HIST_ARENAS), lambda cfg: c1_commands(HIST_ARENAS, 5 * HIST_K, HIST_K),
               HIST_DEPTH, HIST_K, on_at=HIST_K)


def _deep_commands(cfg, k=384, lead=2 * HIST_K):
    """`lead` steps as the other histories (the depth-1 log runs over them), then one launch of 384 steps for depth 64:
    arena 0 ends 192 games in it (3 x depth), arena 1 64, arena 2 63, arena 3 65, arena 4 one, arena 5 none."""
    c = config.bench_commands(HIST_ARENAS, 1, lead + k)[0].copy()
    rotating_schedule(c[:lead], HIST_K)
    lay_quits(c, [2, 6, 0, 0, k, 0, 7, 9], start=lead)
    lay_quits(c, [0, 0, 6, 6, 0, 0, 0, 0], start=lead, stop=lead + k - 6)
    lay_quits(c, [0, 0, 0, 3, 0, 0, 0, 0], start=lead + k - 6)
    return c


DEPTH_1 = Case("C1-depth-1", c1_workload(HIST_ARENAS), lambda cfg: _deep_commands(cfg)[:2 * HIST_K], 1, HIST_K)
DEPTH_64 = Case("C1-depth-64", c1_workload(HIST_ARENAS), _deep_commands, 64, 384, on_at=2 * HIST_K)
NO_RESET_ARENAS = 32


def _no_reset_commands(cfg, k=WIDE_K):
    """auto_reset = 0, two launches of 40 steps: arena a's one game ends at step 8 + 2a (a < 20: inside the first launch,
    then the second), `ind` giving up in the even arenas (DIED) and everybody else in the odd ones (WON); arenas with
    a % 8 == 7 play on."""
    A = NO_RESET_ARENAS
    c = vc.commands(A, 2 * k)[:, :, :cfg.n_agents].copy()
    c[c == QUIT] = ord("x")
    at = [8 + 2 * a for a in range(A)]
    return lay_quits(c, [0 if a % 8 == 7 or a & 1 else at[a] + 1 for a in range(A)],
                     others_at=[at[a] if a & 1 and a % 8 != 7 else None for a in range(A)])


NO_RESET = Case("KITS-no-auto-reset", lambda: config.baseline_workload("KITS", arenas=NO_RESET_ARENAS, auto_reset=0),
                _no_reset_commands, WIDE_DEPTH, WIDE_K)
SEED_TB, SEED_SERIAL = (1 << 32) - 3, (1 << 32) + 5


def _seed(writer):
    return Case("C1-seed-carry-" + writer, c1_workload(4, stride=1), lambda cfg: c1_commands(4, 3 * HIST_K, HIST_K),
                HIST_DEPTH, HIST_K, writer=writer, seeds=lambda w: w.seeds(base_tb=SEED_TB, serial=SEED_SERIAL))


SEEDS = [_seed("launch"), _seed("split")]

ALL = VARIANTS + WRITERS + [RESET_WIDE] + COUNTS + LARGE + [LATE_ON, DEPTH_1, DEPTH_64, NO_RESET] + SEEDS
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)
